"""The beam-search decode (include/qtx.h, beam search) on the GPU against tests/beam_ref.py,
bit for bit: the two per-op kernels on crafted states, the whole decode on every kind of
model and path, and that the greedy decodes are left alone.

Expected values never come from the code under test: the selection is beam_ref.select_ref on
the oracle's log-softmax, the reorder a numpy gather, the decode beam_ref.beam_ref.  Floats are
compared by their bit patterns.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
import model_cfgs as MC  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
NINF = f32(-np.inf)
MAX_LEN = R.MAX_LEN
_MODELS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def call(name, *args):
    from qtx import _lib
    _lib.call(name, *args)


def status(name, *args):
    from qtx import _lib
    return getattr(_lib.lib(), name)(*args)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def gpu_model(d_ff, weight_bits=8, tgt_vocab=97, boosted=True):
    """The QtxModel of one (boosted) small config, built once per process."""
    from qtx.model import QtxModel
    key = (d_ff, weight_bits, tgt_vocab, boosted)
    if key not in _MODELS:
        if boosted:
            cfg, sd, _ = R.boosted_state(d_ff, weight_bits, tgt_vocab)
        elif (d_ff, weight_bits, tgt_vocab) in MC.SEEDS:
            cfg, sd, _ = MC.small_state(d_ff, weight_bits, tgt_vocab)
        else:                       # a vocabulary of the per-op tests only
            from qtx.weights import synthetic_state_dict
            cfg = MC.small_cfg(d_ff, weight_bits, tgt_vocab)
            sd = synthetic_state_dict(1, cfg, ln_random=True)
        _MODELS[key] = QtxModel(sd, cfg)
    return _MODELS[key]


# =====================================================================================
# 1. k_beam_select on crafted states
# =====================================================================================
def scenarios(K, V, seed, eos, pad):
    """[(name, score [K], fin [K], len [K], logits [K, V])]: the rows the selection can meet."""
    rng = np.random.default_rng(seed)
    rows = lambda: (rng.standard_normal((K, V)) * 2).astype(f32)
    live_score = lambda: np.sort((-rng.uniform(0.5, 6, K)).astype(f32))[::-1].copy()
    none, out = np.zeros(K, bool), []
    first = np.full(K, NINF, f32)
    first[0] = 0
    out.append(("first step", first, none, np.zeros(K, np.int32), rows()))
    x = rows()
    sc = live_score()
    if K >= 2:                                   # two slots, identical rows and scores
        x[1] = x[0]
        sc[1] = sc[0]
    out.append(("identical slots", sc, none, np.full(K, 4, np.int32), x))
    x = rows()
    x[:, ::5] = x.max() + f32(0.5)               # repeated values, the maximum among them
    x[0, 3::7] = f32(-1.25)
    out.append(("repeated values", live_score(), none, np.full(K, 4, np.int32), x))
    # a finished slot (the last) whose score ranks first, middle, last, below the cut
    for where in ("first", "middle", "last", "below"):
        x, sc = rows(), live_score()
        fin = none.copy()
        fin[K - 1] = True
        ln = np.full(K, 4, np.int32)
        ln[K - 1] = 2
        if K == 1:
            if where != "first":
                continue
        else:
            lp = O.log_softmax_argmax(x[:K - 1])[0]
            v = np.sort((sc[:K - 1, None] + lp).astype(f32).reshape(-1))[::-1]
            sc[K - 1] = {"first": v[0] + f32(1), "middle": (v[K // 2 - 1] + v[K // 2]) / f32(2),
                         "last": (v[K - 2] + v[K - 1]) / f32(2), "below": v[K - 1] - f32(1)}[where]
        out.append(("finished " + where, sc, fin, ln, x))
    x = rows()
    x[K - 1] = NINF                              # a row of all -inf
    out.append(("row -inf", live_score(), none, np.full(K, 4, np.int32), x))
    x = rows()
    x[K - 1, V // 2] = np.nan                    # a row holding a NaN
    out.append(("row NaN", live_score(), none, np.full(K, 4, np.int32), x))
    x = rows()
    x[0, eos] = x.max() + f32(5)                 # eos wins
    sc = live_score()
    out.append(("eos wins", sc, none, np.full(K, 4, np.int32), x))
    return out


def select_expected(score, fin, ln, logits, s, eos, pad):
    lp = O.log_softmax_argmax(logits)[0]
    par, tok, val = R.select_ref(score, fin, lp, pad)
    pfin = np.asarray(fin)[par]
    nfin = pfin | (tok == eos)
    nlen = np.where(pfin, np.asarray(ln)[par], s + 1).astype(np.int32)
    return par.astype(np.int32), tok.astype(np.int32), val.astype(f32), nfin.astype(np.int32), nlen


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("V", [97, 4444, 8200])
def test_select_op(torch, V, K, B):
    gm = gpu_model(512, 8, V, boosted=False)
    eos, pad, s = R.EOS, R.PAD, 4
    sc_all = scenarios(K, V, 100 + V + K, eos, pad)
    names = [c[0] for c in sc_all]
    assert {"first step", "identical slots", "repeated values", "finished first", "row -inf",
            "row NaN", "eos wins"} <= set(names)
    if K > 1:
        assert {"finished middle", "finished last", "finished below"} <= set(names)
    dev = gm.device
    for c0 in range(0, len(sc_all), B):
        grp = [sc_all[(c0 + i) % len(sc_all)] for i in range(B)]
        score = np.concatenate([g[1] for g in grp]).astype(f32)
        fin = np.concatenate([g[2] for g in grp]).astype(np.int32)
        ln = np.concatenate([g[3] for g in grp]).astype(np.int32)
        logits = np.concatenate([g[4] for g in grp]).astype(f32)
        exp = [select_expected(g[1], g[2], g[3], g[4], s, eos, pad) for g in grp]
        e_par, e_tok, e_val, e_fin, e_len = (np.concatenate([e[i] for e in exp]) for i in range(5))
        Rw = B * K
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t_score, t_fin, t_len, t_logits = d(score), d(fin), d(ln), d(logits)
        t_par = torch.full((Rw,), -7, dtype=torch.int32, device=dev)
        t_bp = torch.full((2, MAX_LEN - 1, Rw), -7, dtype=torch.int32, device=dev)
        t_x = torch.full((Rw, 512), float("nan"), dtype=torch.float32, device=dev)
        t_step = torch.tensor([s, 0, 0, -1], dtype=torch.int32, device=dev)
        call("qtx_beam_select", gm.handle, P(t_logits), B, K, eos, pad, MAX_LEN, P(t_step),
             P(t_score), P(t_fin), P(t_len), P(t_par), P(t_bp[0]), P(t_bp[1]), P(t_x), S0)
        torch.cuda.synchronize()
        tag = f"{[g[0] for g in grp]}"
        np.testing.assert_array_equal(t_par.cpu().numpy(), e_par, tag)
        bp = t_bp.cpu().numpy()
        np.testing.assert_array_equal(bp[0, s], e_par, tag)
        np.testing.assert_array_equal(bp[1, s], e_tok, tag)
        assert (np.delete(bp, s, axis=1) == -7).all(), "a back-pointer row of another step written"
        np.testing.assert_array_equal(bits(t_score.cpu().numpy()), bits(e_val), tag)
        np.testing.assert_array_equal(t_fin.cpu().numpy(), e_fin, tag)
        np.testing.assert_array_equal(t_len.cpu().numpy(), e_len, tag)
        np.testing.assert_array_equal(t_step.cpu().numpy(), [s + 1, 0, 0, int((e_fin == 0).sum())])
        x_exp = gm.embed(d(e_tok.astype(np.int64)[:, None]), "tgt", pos0=s + 1)[:, 0]
        np.testing.assert_array_equal(bits(t_x.cpu().numpy()), bits(x_exp.cpu().numpy()), tag)
        if "eos wins" in tag:
            assert (e_tok == eos).any() and e_fin.any()


# =====================================================================================
# 2. k_beam_reorder on guarded buffers
# =====================================================================================
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("t", [0, 3, 4, MAX_LEN - 2])
@pytest.mark.parametrize("parents", [(0, 1, 2, 3), (0, 0, 2, 1), (3, 3, 3, 3), (1, 2, 0)])
def test_reorder_op(torch, parents, t, grouped, poison):
    reorder_case(torch, parents, t, grouped, poison)


# beam 5 .. 8: all eight of a thread's chunk registers (a shared parent, a dropped slot, cycles)
@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("t", [4, MAX_LEN - 2])
@pytest.mark.parametrize("parents", [(7, 0, 0, 3, 5, 6, 1, 2), (7, 6, 5, 4, 3, 2, 1, 0), (4, 0, 0, 2, 1)])
def test_reorder_op_wide_beam(torch, parents, t, grouped):
    reorder_case(torch, parents, t, grouped, POISONS[0])


def reorder_case(torch, parents, t, grouped, poison, ML=MAX_LEN):
    K, B, L, n = len(parents), 2, 2, t + 1
    Rw = B * K
    krow = ML * 512
    vrow = ((ML + 3) // 4) * 2048 if grouped else ML * 512
    # sentence 0 takes the vector, sentence 1 the same rolled by one (another permutation)
    par = np.array([parents, np.roll(parents, 1)], np.int32).reshape(-1)
    rng = np.random.default_rng(7 * t + K)
    host, devb, checks = {}, {}, []
    for name, row, dt, tdt in (("kc", krow, np.int8, torch.int8), ("vc", vrow, np.int8, torch.int8),
                               ("skc", ML, f32, torch.float32), ("svc", ML, f32, torch.float32)):
        a = (rng.integers(-127, 128, (L, Rw, row)).astype(np.int8) if dt is np.int8
             else rng.standard_normal((L, Rw, row)).astype(f32))
        buf, chk = guarded(torch, (L, Rw, row), tdt, poison, name=name)
        buf.copy_(torch.from_numpy(a))
        host[name], devb[name] = a, buf
        checks.append(chk)
    step = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
    par_d = torch.from_numpy(par).cuda()
    call("qtx_beam_reorder", P(devb["kc"]), P(devb["vc"]), P(devb["skc"]), P(devb["svc"]), B, K, ML,
         L, Rw * krow, Rw * vrow, Rw * ML, grouped, P(step), P(par_d), S0)
    torch.cuda.synchronize()
    src_rows = (np.arange(B)[:, None] * K + par.reshape(B, K)).reshape(-1)
    prefix = {"kc": n * 512, "vc": ((n + 3) // 4) * 2048 if grouped else n * 512, "skc": n, "svc": n}
    for name, a in host.items():
        exp = a.copy()
        exp[:, :, :prefix[name]] = a[:, src_rows, :prefix[name]]      # the moved prefix
        got = devb[name].cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint8 if a.dtype == np.int8 else np.uint32),
                                      exp.view(np.uint8 if a.dtype == np.int8 else np.uint32), name)
    for chk in checks:
        chk()
    np.testing.assert_array_equal(step.cpu().numpy(), [n, 0, 0, 0])


# =====================================================================================
# 3. the whole decode == beam_ref
# =====================================================================================
def gpu_beam(gm, src, mask, beam, early_exit=True, max_len=MAX_LEN):
    from qtx.decode import beam_decode
    r = beam_decode(gm, src, mask, max_len, R.START, beam_size=beam, eos=R.EOS, pad=R.PAD,
                    n_best=beam, early_exit=early_exit)
    assert r.hyp_ids.shape == (src.shape[0], beam, max_len) and r.hyp_ids.dtype == np.int64
    assert r.hyp_score.dtype == f32 and r.hyp_len.dtype == np.int32
    np.testing.assert_array_equal(r.ids, r.hyp_ids)     # length_penalty 0 keeps the order
    return r


def assert_same(r, ref, chunk=8, early=True):
    np.testing.assert_array_equal(r.hyp_ids, ref["hyp_ids"])
    np.testing.assert_array_equal(r.hyp_len, ref["hyp_len"])
    np.testing.assert_array_equal(bits(r.hyp_score), bits(ref["hyp_score"]))
    total = ref["hyp_ids"].shape[-1] - 1
    want = min(total, -(-ref["steps_run"] // chunk) * chunk) if early else total
    assert r.steps_run == want, (r.steps_run, want, ref["steps_run"])


@pytest.mark.parametrize("rows", [None, (1,)], ids=["B4", "B1"])
@pytest.mark.parametrize("d_ff,wbits,V,beam", R.MODELS)
def test_decode_matches_reference(torch, d_ff, wbits, V, beam, rows):
    gm = gpu_model(d_ff, wbits, V)
    src, mask = R.inputs(d_ff, wbits, V)
    if rows is not None:
        src, mask = src[list(rows)], mask[list(rows)]
    assert_same(gpu_beam(gm, src, mask, beam), R.reference(d_ff, wbits, V, beam, rows=rows))


@pytest.mark.parametrize("knob", [None, ("QTX_NO_GRAPH", 1), ("QTX_GRAPH_STEPS", 3),
                                  ("QTX_UNFUSED", 1)], ids=lambda k: "default" if k is None else k[0])
def test_decode_paths(torch, knob_env, knob):
    if knob is not None:
        knob_env(*knob)
    chunk = 3 if knob == ("QTX_GRAPH_STEPS", 3) else 8
    gm = gpu_model(512)
    src, mask = R.inputs()
    ref = R.reference(512, 8, 97, 4)
    assert_same(gpu_beam(gm, src, mask, 4, early_exit=True), ref, chunk, True)
    assert_same(gpu_beam(gm, src, mask, 4, early_exit=False), ref, chunk, False)
    rows = R.early_rows(ref)
    assert rows == (0, 2)
    ref2 = R.reference(512, 8, 97, 4, rows=rows)
    assert ref2["steps_run"] < MAX_LEN - 1
    r2 = gpu_beam(gm, src[list(rows)], mask[list(rows)], 4, early_exit=True)
    assert_same(r2, ref2, chunk, True)
    assert r2.steps_run < MAX_LEN - 1
    assert_same(gpu_beam(gm, src[list(rows)], mask[list(rows)], 4, early_exit=False), ref2, chunk, False)


def test_beam1_against_gpu_greedy(torch):
    from qtx.decode import greedy_decode
    gm = gpu_model(512)
    src, mask = R.inputs()
    ys = greedy_decode(gm, src, mask, MAX_LEN, R.START)
    r = gpu_beam(gm, src, mask, 1)
    seen = 0
    for b in range(src.shape[0]):
        hit = np.nonzero(ys[b, 1:] == R.EOS)[0]
        n = hit[0] + 2 if hit.size else MAX_LEN
        seen += bool(hit.size)
        np.testing.assert_array_equal(r.hyp_ids[b, 0, :n], ys[b, :n])
        assert (r.hyp_ids[b, 0, n:] == R.PAD).all() and r.hyp_len[b, 0] == n - 1
    assert 0 < seen < src.shape[0]


LP = 1.0     # a length penalty that reorders some sentence's hypotheses (asserted below)


def ranked_expected(ref, length_penalty, n_best):
    """(ids, scores float64, lengths) the Python layer must return, from the reference."""
    order = R.rank(ref["hyp_score"], ref["hyp_len"], length_penalty)[:, :n_best]
    s = ref["hyp_score"].astype(np.float64) / np.maximum(ref["hyp_len"], 1) ** float(length_penalty)
    return (np.take_along_axis(ref["hyp_ids"], order[:, :, None], 1),
            np.take_along_axis(s, order, 1), np.take_along_axis(ref["hyp_len"], order, 1))


@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_n_best_length_penalty_torch_input(torch, where):
    """beam_decode with n_best < beam_size, a length penalty that reorders, and torch inputs:
    the ranked outputs are the reference's, and come back as tensors where src lives."""
    from qtx.decode import beam_decode
    gm = gpu_model(512)
    src, mask = R.inputs()
    ref = R.reference(512, 8, 97, 4)
    order = R.rank(ref["hyp_score"], ref["hyp_len"], LP)
    assert (order[:, :2] != np.arange(2)).any(), "the penalty reorders nothing: pick another"
    e_ids, e_sc, e_len = ranked_expected(ref, LP, 2)
    src_t = torch.from_numpy(src).to(where)
    r = beam_decode(gm, src_t, torch.from_numpy(mask).to(where), MAX_LEN, R.START, beam_size=4,
                    eos=R.EOS, pad=R.PAD, length_penalty=LP, n_best=2)
    for a in (r.ids, r.scores, r.lengths, r.hyp_ids, r.hyp_score, r.hyp_len):
        assert torch.is_tensor(a) and a.device == src_t.device
    assert r.ids.shape == (4, 2, MAX_LEN) and r.ids.dtype == torch.int64
    assert r.scores.dtype == torch.float64 and r.lengths.dtype == torch.int32
    np.testing.assert_array_equal(r.ids.cpu().numpy(), e_ids)
    np.testing.assert_array_equal(r.scores.cpu().numpy(), e_sc)
    np.testing.assert_array_equal(r.lengths.cpu().numpy(), e_len)
    np.testing.assert_array_equal(r.hyp_ids.cpu().numpy(), ref["hyp_ids"])
    np.testing.assert_array_equal(bits(r.hyp_score.cpu().numpy()), bits(ref["hyp_score"]))
    with pytest.raises(ValueError):
        beam_decode(gm, src, mask, MAX_LEN, R.START, beam_size=2, n_best=3)


def test_evaluate_with_beam_decoder(torch):
    """data.evaluate through data.beam_decoder: the shared sources as text, two batches; the ids
    scored are the best ranked hypothesis of the reference."""
    from qtx import data as D
    gm = gpu_model(512)
    src, _ = R.inputs()
    vs = D.Vocab(list(D.SPECIALS) + [f"s{i}" for i in range(4, 64)])
    vt = D.Vocab(list(D.SPECIALS) + [f"t{i}" for i in range(4, 97)])
    text = lambda row, v: " ".join(v.itos[x] for x in row[1:] if x not in (R.EOS, R.PAD))
    pairs = [(text(row, vs), "t5 t6 t7") for row in src]
    np.testing.assert_array_equal(D.collate(pairs, vs, vt, src.shape[1])[0], src)
    r = D.evaluate(gm, pairs, vs, vt, batch_size=3, max_padding=src.shape[1], max_len=MAX_LEN,
                   decode=D.beam_decoder(gm, beam_size=4, length_penalty=LP))
    np.testing.assert_array_equal(r.ids, ranked_expected(R.reference(512, 8, 97, 4), LP, 1)[0][:, 0])
    assert len(r.hypotheses) == 4 and 0.0 <= r.bleu <= 1.0
    # default arguments (beam 4, no penalty) on sentences 0 and 2, which stop early
    r2 = D.evaluate(gm, [pairs[0], pairs[2]], vs, vt, batch_size=2, max_padding=src.shape[1],
                    max_len=MAX_LEN, decode=D.beam_decoder(gm))
    np.testing.assert_array_equal(r2.ids, R.reference(512, 8, 97, 4, rows=(0, 2))["hyp_ids"][:, 0])


def test_greedy_untouched(torch):
    """The greedy and the scored decode before and after beam calls on the same model, with
    enough beam shapes in between to roll the 16-entry graph cache."""
    from qtx.decode import greedy_decode
    gm = gpu_model(512)
    src, mask = R.inputs()
    before = greedy_decode(gm, src, mask, MAX_LEN, R.START)
    b_ys, b_sc = greedy_decode(gm, src, mask, MAX_LEN, R.START, return_scores=True)
    np.testing.assert_array_equal(before, R.boosted_state(512)[2].greedy_decode(src, mask, MAX_LEN))
    for ml in range(4, 14):                      # one- and eight-step graphs per shape
        gpu_beam(gm, src, mask, 2, early_exit=False, max_len=ml)
    assert_same(gpu_beam(gm, src, mask, 4), R.reference(512, 8, 97, 4))
    np.testing.assert_array_equal(greedy_decode(gm, src, mask, MAX_LEN, R.START), before)
    a_ys, a_sc = greedy_decode(gm, src, mask, MAX_LEN, R.START, return_scores=True)
    np.testing.assert_array_equal(a_ys, b_ys)
    np.testing.assert_array_equal(a_sc.top_ids, b_sc.top_ids)
    np.testing.assert_array_equal(bits(a_sc.top_logp), bits(b_sc.top_logp))


@pytest.mark.parametrize("case", ["beam0", "beam9", "beam>V", "eos==pad", "ws short"])
def test_refusals(torch, case):
    from qtx.model import to_u8_mask
    from qtx import _lib
    V = 5 if case == "beam>V" else 97
    gm = gpu_model(512, 8, V, boosted=False)
    src, mask = R.inputs()
    B, S = src.shape
    beam = {"beam0": 0, "beam9": 9, "beam>V": 8}.get(case, 4)
    eos, pad = (R.EOS, R.EOS) if case == "eos==pad" else (R.EOS, R.PAD)
    dev = gm.device
    srcd = torch.from_numpy(src).to(dev)
    md = to_u8_mask(mask, dev).reshape(B, S)
    kk = max(beam, 1)
    ids = torch.full((B, kk, MAX_LEN), -7, dtype=torch.int64, device=dev)
    sc = torch.full((B, kk), -7.0, dtype=torch.float32, device=dev)
    ln = torch.full((B, kk), -7, dtype=torch.int32, device=dev)
    nb = int(_lib.lib().qtx_beam_workspace_size(gm.handle, B, S, MAX_LEN, min(max(beam, 1), 8)))
    assert nb > 0
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=dev)
    steps = C.c_int32(-1)
    rc = status("qtx_beam_decode", gm.handle, P(srcd), P(md), B, S, MAX_LEN, beam, R.START, eos,
                pad, 1, P(ids), P(sc), P(ln), C.byref(steps), P(ws),
                nb - 1 if case == "ws short" else nb, S0)
    torch.cuda.synchronize()
    assert rc == (3 if case == "ws short" else 1), _lib.lib().qtx_last_error()
    assert steps.value == -1
    assert (ids == -7).all() and (sc == -7).all() and (ln == -7).all() and (ws == 0x5A).all()
