"""Guards of tests/long_target.py on the CPU: the oracle's own results are what the GPU tests of
the long-target regime (tests/test_gpu_long_target.py) need them to be.  A long decode that
repeats one token would pass with a stuck cache or a frozen key count, a fault that changes
nothing with a kernel that ignores it, and a beam search that ends early never reorders a
cache past position 128.  Everything here is the oracle; results are memoised in long_target.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_target as LT  # noqa: E402

IDS = [LT.cfg_id(c) for c in LT.CONFIGS]


@pytest.mark.parametrize("c", LT.CONFIGS, ids=IDS)
def test_decode_is_not_degenerate_past_128(c):
    """Some sentence holds at least 3 distinct tokens at the positions 129 and up (per case,
    not per sentence: a sentence may collapse to one token)."""
    ys, ti, tv = LT.scored(c)
    assert ys.shape == (LT.B, LT.L) and ti.shape == tv.shape == (LT.B, LT.L - 1, 2)
    assert LT.tail_distinct(ys) >= 3, ys[:, 129:]
    assert np.isfinite(tv).all()


def test_models_share_model_cfgs_weights():
    """The 192- and 512-row-table models hold model_cfgs.small_state's weights where the seeds
    agree; only the positional table differs."""
    import model_cfgs as MC
    sd = LT.state(512, 8)[1]
    ref = MC.small_state(512, 8)[1]
    cap = LT.state(512, 8, LT.CAP_ROWS)[1]
    for k, v in ref.items():
        if not k.endswith(".pe"):
            np.testing.assert_array_equal(sd[k], v)
            np.testing.assert_array_equal(cap[k], v)
    assert sd["tgt_embed.1.pe"].shape[1] == LT.PE_ROWS and cap["tgt_embed.1.pe"].shape[1] == LT.CAP_ROWS
    np.testing.assert_array_equal(cap["tgt_embed.1.pe"][:, :LT.PE_ROWS], sd["tgt_embed.1.pe"])


@pytest.mark.parametrize("c", [(512, 8), (1024, 8)], ids=IDS[:2])
def test_full_pass_reproduces_the_cached_decode(c):
    """Causal invariance in the oracle at T = 139: the teacher-forced pass over the decode's
    prefix picks the cached decode's token at every position."""
    np.testing.assert_array_equal(LT.full_pass_tokens(c), LT.scored(c)[0][:, 1:])


def test_masks_and_long_source_are_what_they_claim():
    tm = LT.pad_mask()
    assert tm.shape == (LT.B, LT.T_FULL, LT.T_FULL) and tm.dtype == np.uint8
    causal = np.tril(np.ones((LT.T_FULL, LT.T_FULL), np.uint8))
    assert (tm <= causal[None]).all()
    for b in range(LT.B):                       # holes below and above position 128
        dropped = np.nonzero(tm[b, -1] == 0)[0]
        assert (dropped < 128).any() and (dropped >= 128).any()
    assert not tm[1, 133].any() and tm[1, 132].any() and tm[1, 134].any() and tm[0, 133].any()
    assert not np.array_equal(tm[0], tm[1])     # a mask per sentence: the batch stride matters
    src, m = LT.long_inputs()
    assert src.shape == (2, LT.LONG_S) and m.sum(-1).reshape(-1).tolist() == list(LT.LONG_LENS)
    src, m = LT.inputs()
    assert m[0].all() and not m[1].all()


def test_padded_pass_differs_from_the_causal_one():
    c = (512, 8)
    a, b = LT.full_pass(c)["out"], LT.full_pass(c, "padded")["out"]
    assert a.shape == b.shape == (LT.B, LT.T_FULL, 512)
    assert not np.array_equal(a[0, 129:], b[0, 129:]) and not np.array_equal(a[1, 129:], b[1, 129:])
    assert np.isfinite(b).all()                 # the fully masked row: a uniform softmax, no NaN


def test_score_of_the_decode_is_rank_zero():
    c = (512, 8)
    ys, ti, tv = LT.scored(c)
    ref = LT.score_golden(c)
    assert (ref["rank"] == 0).all()
    np.testing.assert_array_equal(ref["top_ids"], ti)
    np.testing.assert_array_equal(ref["top_logp"], tv)
    np.testing.assert_array_equal(ref["tok_logp"], tv[..., 0])
    tgt, pref = LT.score_padded(c)
    assert (tgt[1, list(LT.PAD_AT)] == 2).all() and min(LT.PAD_AT) > 128
    # the pad-aware mask changes what the positions behind the first pad see
    first = min(LT.PAD_AT)
    assert not np.array_equal(pref["top_logp"][1, first:], ref["top_logp"][1, first:])
    np.testing.assert_array_equal(pref["top_logp"][0], ref["top_logp"][0])


def test_fault_golden_is_the_scored_decode():
    """kvfault_ref.golden (the state before each step, for the fault cases) is the oracle's
    scored decode."""
    g, (ys, ti, tv) = LT.kv_golden(), LT.scored(LT.FAULT_CFG)
    np.testing.assert_array_equal(g["ys"], ys)
    np.testing.assert_array_equal(g["top_ids"], ti)
    np.testing.assert_array_equal(g["top_logp"], tv)


@pytest.mark.parametrize("name", sorted(LT.dfault_trials()))
def test_dfault_trial_changes_a_token(name):
    """The faulty pass at T = 134 changes the token of step 133 in some sentence, so the steps
    134 .. 138 run again on the changed prefix."""
    f = LT.dfault_trials()[name]
    assert f.module == 1
    if f.linear == "QK":
        assert f.row % LT.DF_T == 130
    if f.linear == "PV":
        assert f.col % LT.DF_T == 131
    ys, ti, tv, rec = LT.dfault_trial(name)
    gold = LT.kv_golden()["ys"]
    changed = rec[0][:, 0] != rec[2][:, 0]
    assert changed.any(), name
    np.testing.assert_array_equal(ys[:, :LT.DF_T], gold[:, :LT.DF_T])
    np.testing.assert_array_equal(ys[:, LT.DF_T] != gold[:, LT.DF_T], changed)
    np.testing.assert_array_equal(ys[~changed], gold[~changed])


@pytest.mark.parametrize("name", sorted(LT.kvfault_cases()))
def test_kvfault_case_changes_tokens(name):
    f, u, step = LT.kvfault_cases()[name]
    assert step > 128
    if u is not None:
        assert u.row % LT.L >= 128 and u.row % LT.L < step
    elif f.linear in ("QK", "PV"):
        j = (f.row if f.kind.startswith("WEIGHT") else f.col) % (step + 1)
        assert j >= 128
    exp = LT.kvfault_trial(name)
    gold = LT.kv_golden()["ys"]
    np.testing.assert_array_equal(exp[0][:, :step + 1], gold[:, :step + 1])
    assert LT.kvfault_effect(name) == "tokens", name
    if name == "out_k_s131":
        # the faulty K row persists: with the fault the step's token may stay, but the rows
        # read later differ, so some LATER token differs
        assert (exp[0][:, step + 2:] != gold[:, step + 2:]).any()


@pytest.mark.parametrize("c", LT.BEAM_CONFIGS, ids=IDS[:2])
def test_beam_reorders_past_128(c):
    """The search runs every step, reorders the caches (a non-identity parent vector) at some
    step >= 129, and some hypothesis is still live past step 135."""
    r = LT.beam_reference(c)
    assert r["steps_run"] == LT.L - 1
    par, fins = np.stack(r["parents"]), np.stack(r["fins"])
    late = [s for s in range(129, len(par)) if (par[s] != np.arange(LT.BEAM)).any()]
    assert late, "no reorder at a step >= 129"
    assert not fins[136].all()
    # the hypotheses of a sentence differ past 128
    hyp = r["hyp_ids"]
    assert any((hyp[b, 0, 129:] != hyp[b, k, 129:]).any() for b in range(LT.B) for k in (1, 2))
    # d_ff 1024: final hypotheses descend through cache rows moved at steps >= 129 and read
    # again later, so a reorder that stops at 128 positions changes their tokens or scores.
    # The d_ff 512 model repeats one token whatever the EOS bias (tried -1 .. 1.5): its best
    # hypothesis keeps slot 0 and the others are its fresh children at every step, whose moved
    # rows no surviving hypothesis reads; that search pins the carving, the tail and steps_run.
    moves = LT.beam_late_moves(r)
    assert moves or c != (1024, 8)
