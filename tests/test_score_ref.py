"""Teacher-forced target scoring on the CPU: the contract of tests/score_ref.py against the
oracle's KV-cached steps and torch, what the shared fixture exercises (asserted per model, so
that the GPU tests in tests/test_gpu_score.py compare more than rank-0 rows and fault-free
passes), and the host arithmetic of qtx.decode / qtx.data."""
import math

import numpy as np
import pytest

import beam_ref as BR
import score_ref as SR
from oracle import qtx_oracle as O

f32 = np.float32


@pytest.mark.parametrize("cfg", SR.MODELS, ids=str)
def test_greedy_ids_score_rank0_and_equal_the_cached_steps(cfg):
    """Scoring the oracle's own greedy ids: every label is the first choice, its log-prob the
    top one, and the full-prefix pass's log-probabilities are the KV-cached steps' bit for bit."""
    om = SR.model(*cfg)[2]
    src, mask = SR.inputs()
    g, gs = SR.greedy(*cfg), SR.greedy_scores(*cfg)
    assert (gs["rank"] == 0).all()
    np.testing.assert_array_equal(gs["tok_logp"], gs["top_logp"][..., 0])
    np.testing.assert_array_equal(gs["top_ids"][..., 0], g[:, 1:])
    st = O.DecodeState(om, om.encode(om.embed(src, om.src_lut), mask), mask, SR.L)
    for t in range(SR.L - 1):
        logp = O.log_softmax_argmax(om.logits(st.step(om.embed(g[:, t:t + 1], om.tgt_lut, pos0=t))))[0]
        np.testing.assert_array_equal(logp, gs["logp"][:, t])


@pytest.mark.parametrize("cfg", SR.MODELS, ids=str)
def test_fixture_exercises_ranks_and_padding(cfg):
    tgt = SR.targets(*cfg)
    ref = SR.reference(*cfg)
    m = tgt[:, 1:] != SR.PAD
    assert (ref["rank"][:, :3] == 0).all() and (ref["rank"][:, 3] == 1).all()   # by construction
    assert (ref["rank"][m] >= 2).any()
    assert (~m).any(-1).sum() == 2 and m.all(-1).sum() == 1     # two padded sentences, one full
    # the pad-aware mask equals the causal one on every row whose label is not pad, bit for
    # bit, and differs on some pad-label row
    plain = SR.reference(*cfg, pad=-1)
    np.testing.assert_array_equal(ref["logp"][m], plain["logp"][m])
    assert not np.array_equal(ref["logp"][~m], plain["logp"][~m])
    assert np.isfinite(ref["tok_logp"]).all()


def test_chosen_faults_change_what_they_should():
    cfg = SR.MODELS[0]
    gold = SR.reference(*cfg)
    trials = [SR.reference(*cfg, fault=f) for f in SR.faults()]
    assert trials[0]["tok_logp"].tobytes() != gold["tok_logp"].tobytes()   # the encoder fault
    assert any((t["tok_logp"] != gold["tok_logp"]).any() for t in trials[1:])
    assert any((t["rank"] != gold["rank"]).any() for t in trials)
    for t in trials:                        # every trial differs from golden somewhere
        assert t["logp"].tobytes() != gold["logp"].tobytes()


@pytest.mark.parametrize("V", [2, 97, 4444])
def test_rule_on_crafted_rows(V):
    torch = pytest.importorskip("torch")
    x, y = SR.crafted_rows(V)
    tok, rank, ti, tv = SR.score_logits(x, y)
    names = ["equal", "two_max", "ulp", "nan", "inf", "all_ninf", "first", "last", "above",
             "below", "ninf_label", "argmax"]
    k = {n: i for i, n in enumerate(names)}
    assert rank[k["equal"]] == V - 1 and tuple(ti[k["equal"]]) == (0, 1)
    assert rank[k["two_max"]] == 1 and tuple(ti[k["two_max"]]) == (0, V - 1)
    assert tv[k["two_max"], 0] == tv[k["two_max"], 1] == tok[k["two_max"]]
    assert tuple(ti[k["ulp"]]) == (V - 1, 0) and rank[k["ulp"]] == 1
    for n in ("nan", "inf", "all_ninf"):
        assert np.isnan(tok[k[n]]) and rank[k[n]] == -1 and tuple(ti[k[n]]) == (0, 1)
        assert np.isnan(tv[k[n]]).all()
    for n in ("above", "below"):            # the label out of range: the top 2 still the row's
        assert np.isnan(tok[k[n]]) and rank[k[n]] == -1 and np.isfinite(tv[k[n]]).all()
    assert rank[k["argmax"]] == 0 and tok[k["argmax"]] == tv[k["argmax"], 0]
    if V > 2:
        assert rank[k["ninf_label"]] == V - 1 and tok[k["ninf_label"]] == -np.inf
    # against torch wherever the values are distinct
    fin = [k[n] for n in ("ulp", "first", "last", "argmax", "above", "below")]
    lp = O.log_softmax_argmax(x[fin])[0]
    tl = torch.log_softmax(torch.from_numpy(x[fin]).double(), -1).numpy()
    np.testing.assert_allclose(lp, tl, rtol=0, atol=2e-6 * (1 + np.abs(tl).max()))
    vals, idx = torch.topk(torch.from_numpy(lp), 2, dim=-1)
    np.testing.assert_array_equal(vals.numpy(), tv[fin])
    distinct = vals[:, 0] != vals[:, 1]
    np.testing.assert_array_equal(idx.numpy()[distinct], ti[fin][distinct])
    for j, i in enumerate(fin):
        if 0 <= y[i] < V and len(np.unique(lp[j])) == V:
            assert rank[i] == int((lp[j] > lp[j, y[i]]).sum())


def test_target_scores_properties():
    from qtx.decode import TargetScores
    lp = np.array([[-0.5, -1.5, -9.0], [-0.25, -2.0, -0.125]], f32)
    rank = np.array([[0, 3, 0], [1, 0, 0]], np.int32)
    labels = np.array([[5, 1, 2], [7, 8, 1]], np.int64)
    ts = TargetScores(lp, rank, None, None, labels, pad=2)
    assert ts.mask.tolist() == [[True, True, False], [True, True, True]]
    assert ts.n_tokens.tolist() == [2, 3]
    np.testing.assert_array_equal(ts.sentence_logp, np.array([-2.0, -2.375], np.float64))
    assert ts.sentence_logp.dtype == np.float64
    assert ts.hits.tolist() == [[True, False, False], [False, True, True]]
    assert TargetScores(lp, rank, None, None, labels, pad=-1).mask.all()
    # a leading trial axis broadcasts against the [R, T] labels
    t3 = TargetScores(np.stack([lp, lp * 2]), np.stack([rank, rank]), None, None, labels, pad=2)
    np.testing.assert_array_equal(t3.sentence_logp, np.array([[-2.0, -2.375], [-4.0, -4.75]]))
    assert t3.hits.shape == (2, 2, 3)
    torch = pytest.importorskip("torch")
    tt = TargetScores(torch.from_numpy(np.stack([lp, lp * 2])), torch.from_numpy(np.stack([rank, rank])),
                      None, None, torch.from_numpy(labels), pad=2)
    np.testing.assert_array_equal(tt.sentence_logp.numpy(), t3.sentence_logp)
    assert tt.hits.numpy().tolist() == t3.hits.tolist() and tt.n_tokens.tolist() == [2, 3]


def test_rescore_accumulation_reproduces_the_beam_scores():
    """Scoring beam_ref's hypotheses teacher-forced (tgt_per_src = beam) and adding the label
    log-probs sequentially in float32 over t < hyp_len gives hyp_score bit for bit."""
    from qtx.decode import accumulate_logp
    d_ff, wb, V, beam = BR.MODELS[0]
    ref = BR.reference(d_ff, wb, V, beam)
    om = BR.boosted_state(d_ff, wb, V)[2]
    src, mask = BR.inputs(d_ff, wb, V)
    B, K, L = ref["hyp_ids"].shape
    assert np.isfinite(ref["hyp_score"]).all()
    sc = SR.score_ref(om, src, mask, ref["hyp_ids"].reshape(B * K, L), pad=BR.PAD, tgt_per_src=K)
    got = accumulate_logp(sc["tok_logp"], ref["hyp_len"].reshape(-1)).reshape(B, K)
    assert got.dtype == f32
    np.testing.assert_array_equal(got, ref["hyp_score"])


def test_perplexity_arithmetic():
    """data.perplexity with an oracle-backed score callable == a direct computation."""
    from qtx import data
    from qtx.decode import TargetScores
    cfg = SR.MODELS[0]
    om = SR.model(*cfg)[2]
    words_s = [f"s{i}" for i in range(60)]
    words_t = [f"t{i}" for i in range(93)]
    vs, vt = data.Vocab(list(data.SPECIALS) + words_s), data.Vocab(list(data.SPECIALS) + words_t)
    rng = np.random.default_rng(3)
    pairs = [(" ".join(rng.choice(words_s, int(rng.integers(2, 7)))),
              " ".join(rng.choice(words_t, int(rng.integers(1, 8))))) for _ in range(5)]
    calls = []

    def score(s, m, t):
        calls.append(t.shape)
        r = SR.score_ref(om, s, m, t, pad=SR.PAD)
        return TargetScores(r["tok_logp"], r["rank"], None, None, t[:, 1:], pad=SR.PAD)
    res = data.perplexity(None, pairs, vs, vt, batch_size=3, max_padding=12, score=score)
    src, tgt = data.collate(pairs, vs, vt, 12)
    assert [c[0] for c in calls] == [3, 2]
    assert all(c[1] == (tgt[i:i + 3] != SR.PAD).sum(-1).max() for c, i in zip(calls, (0, 3)))
    full = SR.score_ref(om, src, (src != SR.PAD)[:, None, :], tgt, pad=SR.PAD)   # untrimmed
    m = tgt[:, 1:] != SR.PAD
    sent = np.array([math.fsum(r[k].astype(np.float64)) for r, k in zip(full["tok_logp"], m)])
    np.testing.assert_array_equal(res.sentence_logp, sent)
    assert res.n_tokens == int(m.sum())
    assert res.nll == -math.fsum(sent)
    assert res.ppl == float(np.exp(res.nll / res.n_tokens))
    assert res.token_accuracy == int(((full["rank"] == 0) & m).sum()) / int(m.sum())
