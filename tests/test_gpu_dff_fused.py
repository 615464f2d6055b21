"""The fused decode step at every feed-forward width between the flagship ones, d_ff = 256, 768,
1024, 1280, 1536, 1792 (csrc/qtx_decode_dff.hip: k_skinny8_dff, k_skinny at the new K; the gate
fused_step_ok in csrc/qtx_api.hip) against the oracle, bit for bit.

1. FFN2 per op (qtx_skinny_linear, N = 512, residual): M = 1 and 5 run k_skinny8_dff (5: a
   ragged second block), M = 33 k_skinny's 4-row blocks, M = 97 its 8- / 16-row blocks; at three
   K also without the residual flag and with N = 48.  Every case in guarded buffers at both
   alignments (test_gpu_bounds.py's gb fixture).
2. Plain, scored and beam decodes of the two-layer models on every path, with capture counts.
3. The fault drivers (kvfault, cached dfault, kvtrials) at d_ff 768 (odd q) and 1024: their
   golden steps are now the fused step, the faulty step stays eager.
Expected values come from the oracle and the existing reference modules alone."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import dfault_cases as D  # noqa: E402
import kvfault_ref as R  # noqa: E402
import model_cfgs as MC  # noqa: E402
import test_gpu_kvfault as KV  # noqa: E402
import test_gpu_kvtrials as KT  # noqa: E402
from guarded import POISONS  # noqa: E402
from test_gpu_beam import assert_same, gpu_beam  # noqa: E402
from test_gpu_bounds import GB_PARAMS, _skinny_ref, _skinny_run, assert_ok, gb, np_  # noqa: E402,F401
from test_gpu_dfault_cached import cached, check_scored  # noqa: E402
from test_gpu_long_fused import stats  # noqa: E402
from test_gpu_model_configs import GR_L, greedy_case  # noqa: E402
from test_gpu_scored import gpu_scored, torch  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
KS = (256, 768, 1024, 1280, 1536, 1792)
L = 8     # the fault drivers' max_len


# =====================================================================================
# 1. FFN2 per op
# =====================================================================================
def ffn2_ref(amode, M, K, oracle_model, N=512):
    """_skinny_ref's case with two sets of values planted.  x: the absmax of even rows at column
    0, of odd rows at column K - 1 (a half-row maximum that misses the other half changes the
    scale; the all-zero last row stays).  W: row n carries code 1 + (n + 5 s) % 127 — nonzero,
    different for every k-step s of the row — in the last 16 columns of each 64-column k-step
    (a k-step dealt to no wave, or to two, changes the sum)."""
    r = dict(_skinny_ref(amode, M, N, K, 8, oracle_model))
    x, qw = r["x"].copy(), r["qw"].copy()
    top = 2 * np.abs(x).max(-1)
    x[0::2, 0], x[1::2, K - 1] = top[0::2], -top[1::2]
    n, s = np.arange(N)[:, None, None], np.arange(K // 64)[None, :, None]
    qw.reshape(N, K // 64, 64)[:, :, 48:] = 1 + (n + 5 * s) % 127
    r["x"], r["qw"] = x, qw
    r["qx"], r["sx"] = O.quant_rows(x)
    if amode == 2:
        r["parts"] = np.stack([np.abs(c).max(-1) for c in np.array_split(x, r["n"], axis=1)]).astype(f32)
    r["acc"] = O.int_gemm(r["qx"], qw)
    return r


def _gb_cases(cases):
    """(argvalues, ids) of `cases` under each parameter of test_gpu_bounds.py's gb fixture (both
    poisons at 256-byte alignment, 16 (mod 256) under the first).  The first parameter is what
    these tests ran with before they took the fixture, and keeps their ids."""
    vals, ids = [], []
    for (poison, skew), gid in zip(GB_PARAMS, ("", "poison5A-", "align16-poisonA5-")):
        assert (poison, skew) == {"": (POISONS[0], 0), "poison5A-": (POISONS[1], 0),
                                  "align16-poisonA5-": (POISONS[0], 16)}[gid]
        for c, cid in cases:
            vals.append(((poison, skew),) + tuple(c))
            ids.append(gid + cid)
    return vals, ids


# the full M x amode x K product with the step's epilogue (residual, N = 512); no epilogue flag
# (k_skinny<.., 0> at every M: the 8-wave kernel takes the residual form only) and N = 48 (three
# column blocks) at the narrowest K, an odd K / 256 and the widest K
FFN2_CASES = [((K, amode, M, 2, 512), "%d-%d-%d" % (K, amode, M))
              for K in KS for amode in (3, 2, 0) for M in (1, 5, 33, 97)]
FFN2_CASES += [((K, amode, M, flags, N), "%d-%d-%d-flags%d-N%d" % (K, amode, M, flags, N))
               for flags, N in ((0, 512), (0, 48), (2, 48)) for K in (256, 768, 1792)
               for amode in (3, 2, 0) for M in (1, 5, 33, 97)]
_FFN2 = _gb_cases(FFN2_CASES)


@pytest.mark.parametrize("gb,K,amode,M,flags,N", _FFN2[0], ids=_FFN2[1], indirect=["gb"])
def test_ffn2(gb, oracle_model, K, amode, M, flags, N):
    """Every case at both alignments and under both poisons (the gb fixture).  flags 0: the
    residual is still passed and must not reach the result."""
    r = ffn2_ref(amode, M, K, oracle_model, N)
    rc, out, pm = _skinny_run(gb, r, amode, M, N, K, 8, flags)
    assert_ok(rc, "qtx_skinny_linear")
    gb.check()
    y = O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"], relu=False)
    if flags & 2:
        y = r["res"] + y
    np.testing.assert_array_equal(np_(out), y)
    gb.assert_poison(pm, "pmax_out")


_REFUSALS = _gb_cases([((amode, bits, flags), "%d-%d-%d" % (amode, bits, flags))
                       for amode, bits, flags in [(1, 8, 2), (3, 4, 2), (3, 8, 1), (0, 8, 5)]])


@pytest.mark.parametrize("gb,amode,bits,flags", _REFUSALS[0], ids=_REFUSALS[1], indirect=["gb"])
def test_ffn2_refusals(gb, oracle_model, amode, bits, flags):
    """What include/qtx.h excludes at the new K: the LayerNorm prologue, 4-bit weights, the ReLU
    and row-maximum epilogues — QTX_E_UNSUPPORTED, nothing written."""
    r = dict(_skinny_ref(3, 5, 512, 768, 8, oracle_model))
    rc, out, pm = _skinny_run(gb, r, amode, 5, 512, 768, bits, flags)
    assert rc == 4
    gb.check()
    gb.assert_poison(out, "out")
    gb.assert_poison(pm, "pmax_out")


# =====================================================================================
# 2. decodes
# =====================================================================================
def fresh(d_ff, state=MC.small_state):
    from qtx.model import QtxModel
    cfg, sd, om = state(d_ff, 8, 97)
    gm = QtxModel(sd, cfg)
    gm.workspace(64 << 20)        # sized once: every call carves the same memory
    return gm, om


def decode_both(gm, case, max_len):
    from qtx.decode import greedy_decode
    src, m, ys, ti, tv = case
    np.testing.assert_array_equal(greedy_decode(gm, src, m, max_len, 0), ys)
    gy, gi, gv = gpu_scored(gm, src, m, max_len)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)


@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_GRAPH_STEPS": 4}],
                         ids=["default", "no_graph", "graph_steps_4"])
@pytest.mark.parametrize("d_ff", KS)
def test_greedy_and_scored(torch, knob_env, d_ff, env):
    """B = 3.  Default path: the decodes run on graphs of the fused step — at least one capture
    by the first round, none by the second (the parent commit decodes these models eagerly)."""
    for k, v in env.items():
        knob_env(k, v)
    gm, om = fresh(d_ff)
    case = greedy_case((d_ff, 8, 97), om)
    seen = []
    for _ in range(2):
        decode_both(gm, case, GR_L)
        seen.append(stats(gm))
    if not env:
        assert seen[0][1] >= 1 and seen[1] == seen[0], seen


@pytest.mark.parametrize("d_ff,B", [(1280, 33), (768, 100), (1024, 100)])
def test_greedy_more_rows(torch, d_ff, B):
    """B = 33: k_skinny's 4-row blocks with the fp32 prologue; B = 100: the >= 96-row path (the
    hidden quantized by its own kernel, the int8 FFN2 in 16-row blocks)."""
    gm, om = fresh(d_ff)
    decode_both(gm, greedy_case((d_ff, 8, 97), om, B=B, S=9, L=5), 5)
    assert stats(gm)[1] >= 1


def test_beam_is_fused(torch):
    """beam 4 at d_ff 1024 == beam_ref, on captured graphs."""
    gm, _ = fresh(1024, BR.boosted_state)
    src, m = BR.inputs(1024, 8, 97)
    seen = []
    for _ in range(2):
        assert_same(gpu_beam(gm, src, m, 4), BR.reference(1024, 8, 97, 4))
        seen.append(stats(gm))
    assert seen[0][1] >= 1 and seen[1] == seen[0], seen


# =====================================================================================
# 3. fault drivers
# =====================================================================================
TOKEN = {768: (0, 0, 2), 1024: (1, 0, 1)}     # (layer, sentence, step), found on the oracle


def fault_src(d_ff):
    """Its own sentences per model: the reference modules memoise by tag or by source."""
    return MC.small_src(3, 9, d_ff, full=(0,))


def fault_inputs(d_ff):
    """(tag, (src, mask), max_len) in test_gpu_kvfault's form, and the trials: two step faults on
    FFN2's INPUT at the hidden's last column — the first changes a token (TOKEN) — and a cache
    upset."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    layer, b, step = TOKEN[d_ff]
    trials = [(F("INPUT", 1, layer, "FFN2", row=b, col=d_ff - 1, bit=7), None, step),
              (F("INPUT", 1, 1 - layer, "FFN2", row=2, col=d_ff - 1, bit=6), None, 4),
              (None, U("self_v", 1, row=2 * L + 1, col=70, bit=7), 3)]
    return ("dff%d" % d_ff, fault_src(d_ff), L), trials


@pytest.mark.parametrize("d_ff", [768, 1024])
def test_kvfault(torch, d_ff):
    gm, om = fresh(d_ff)
    inp, trials = fault_inputs(d_ff)
    effects = [R.effect(om, inp[1][0], inp[1][1], L, inp[0], KV.check(gm, om, f, u, s, inp))
               for f, u, s in trials]
    assert effects[0] == "tokens" and "none" not in effects, effects


@pytest.mark.parametrize("d_ff", [768, 1024])
def test_dfault_cached(torch, d_ff):
    """The cached decoder-fault decode: golden fused steps, the faulty pass at position 3, then
    fused steps again to the end."""
    from qtx.fault import Fault
    gm, om = fresh(d_ff)
    src_m, tin = fault_src(d_ff), 3
    f = Fault("OUTPUT", 1, 1, "FFN2", row=1 * tin + tin - 1, col=7, value=3.0e4)
    exp = D.oracle_trial(om, src_m[0], src_m[1], L, f, tin, "dff%d" % d_ff)
    assert D.changed(exp)
    check_scored(cached(gm, f, tin, True, src_m, L), exp, tin, L)
    np.testing.assert_array_equal(cached(gm, f, tin, False, src_m, L), exp[0])


@pytest.mark.parametrize("d_ff", [768, 1024])
def test_kvtrials(torch, d_ff):
    """One table of B = 8: step faults and upsets side by side, a row without a trial."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    gm, om = fresh(d_ff)
    src3, m3 = fault_src(d_ff)
    idx = list(KT.SENT)
    src, m = src3[idx], m3[idx]
    hi, lo = (F("INPUT", 1, l, "FFN2", row=0, col=d_ff - 1, bit=b) for l, b in ((1, 7), (0, 6)))
    trials = [(hi, 2), (U("self_v", 1, row=1, col=70, bit=7), 3), None, (lo, 4), (hi, 5), None,
              (lo, 1), (U("cross_k", 0, row=3, col=5, bit=7), 4)]     # (rows: one sentence's own)
    exp = KT.check(gm, om, src, m, trials, L)
    changed = KT.changed_rows(om, src, m, exp, L)
    assert changed and set(changed) <= {b for b, t in enumerate(trials) if t is not None}
