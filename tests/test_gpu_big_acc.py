"""Integer GEMM accumulators of magnitude 2^24 and above, every path that carries one,
bit for bit against the oracle.

The contract is y = ((float(acc) * s_a) * s_w) + b.  Below 2^24 float(acc) is
exact, and random codes never leave that range (tests/test_big_acc_ref.py); the operands of
tests/big_acc.py put every accumulator in [2^24, 2^25), about half of them odd and therefore
exact ties of the conversion, half of them negative.  The oracle converts with
astype(float32): round-to-nearest-even.  A kernel that truncates, rounds half away, or sums
int32 partials in fp32 differs on about a quarter of all outputs.

Outputs sit in guarded buffers (one poison: the two-poison argument is test_gpu_bounds.py's),
inputs are plain allocations.  4-bit weights cannot reach the regime (7 * 127 * 2048 < 2^24),
so there is no 4-bit case.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_acc as BA  # noqa: E402
from guarded import POISONS  # noqa: E402
from test_gpu_bounds import (Guards, P, S0, _rows_operands, _skinny_run, assert_kp,  # noqa: E402,F401
                             assert_ok, call, lib, np_, rows_call, to_kp, torch)
from test_gpu_rowfault_gemm import F, c_table, restate  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
RELU, RESID = 1, 2
_MEMO = {}


@pytest.fixture
def gb(torch):
    return Guards(torch, POISONS[0])


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def case(M, N, K):
    """Crafted codes of one shape with random scales, bias and residual; acc from the oracle."""
    def make():
        lo, flip = BA.PARAMS[K]
        qx, qw = BA.operands(BA.SEED, M, N, K, lo, flip)
        rng = np.random.default_rng(M * 7919 + N + K)
        sx = (rng.random(M) * 0.02 + 0.001).astype(f32)
        sw = (rng.random(N) * 0.002 + 0.0001).astype(f32)
        b = rng.standard_normal(N).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
        acc = O.int_gemm(qx, qw)
        st = BA.stats(acc)
        assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24 and st["odd_big"] >= 0.25
        return dict(qx=qx, sx=sx, qw=qw, sw=sw, b=b, res=res, acc=acc)
    return memo((M, N, K), make)


def fp32_case(M, N, K):
    """The same codes as x = code * 2^-4 for the fp32 prologues: the row scale is 2^-4."""
    def make():
        r = dict(case(M, N, K))
        r["x"] = BA.as_fp32(r["qx"])
        q, s = O.quant_rows(r["x"])
        assert np.array_equal(q, r["qx"]) and (s == BA.X_SCALE).all()
        r["sx"] = s
        return r
    return memo(("f32", M, N, K), make)


# =====================================================================================
# qtx_linear_i8
# =====================================================================================
@pytest.mark.parametrize("M,N,K,flags", [
    (37, 64, 2048, 0),           # the 32-tile k_gemm (M < 256)
    (37, 64, 2048, RESID),
    (257, 272, 2048, RELU),      # k_gemm256 (M >= 256, K % 256 == 0)
    (37, 64, 1280, 0),           # K = 1280: the smallest model K above 1041
    (257, 272, 1344, RESID)])    # the 128-tile k_gemm (M >= 256, K % 256 != 0)
def test_linear_i8(gb, M, N, K, flags):
    r = case(M, N, K)
    out = gb.new((M, N), f32, "out")
    call("qtx_linear_i8", P(gb.dev(r["qx"])), P(gb.dev(r["sx"])), P(gb.dev(r["qw"])),
         P(gb.dev(r["sw"])), P(gb.dev(r["b"])), M, N, K, 8, flags,
         P(gb.dev(r["res"])) if flags & RESID else S0, P(out), S0)
    gb.check()
    y = O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"], relu=bool(flags & RELU))
    got = np_(out)
    if flags & RELU:             # the large negative half is exactly zero, the rest is not
        assert (got[:, 1::2] == 0).all() and (got[:, 0::2] > 0).all()
    np.testing.assert_array_equal(got, r["res"] + y if flags & RESID else y)


# =====================================================================================
# qtx_linear_rows: residual + LayerNorm + quantize over a K = 2048 GEMM
# =====================================================================================
def _rows_expect(r, oracle_model):
    la, lb = oracle_model.dec[1]["ln"][0]
    y = O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"])
    x = r["res"] + y
    ln = O.layer_norm(x, la, lb)
    q, s = O.quant_rows(ln)
    return la, lb, x, ln, q, s


@pytest.mark.parametrize("M,kp,ksplit", [(7, 0, 0), (7, 1, 0), (7, 1, 4), (129, 0, 0), (129, 1, 0),
                                         (129, 1, 4)])
@pytest.mark.parametrize("lnq", [True, False])
def test_linear_rows_res_ln(gb, oracle_model, knob_env, M, kp, ksplit, lnq):
    """k_gemm_row plain (kp 0) and KP (kp 1); ksplit 4: the K split with its int32 partials
    in `part` (RE_PARTIAL) and the row-wise epilogue that sums them, as
    test_gpu_bounds.py::test_linear_rows_splitk_part reaches it; the unsplit KP call also runs
    with QTX_NO_SPLITK=1, the switch the model uses to take it."""
    r = memo(("rows", M), lambda: dict(case(M, 512, 2048)))
    la, lb, x, ln, q, s = memo(("rows-exp", M), lambda: _rows_expect(r, oracle_model))
    if kp == 1 and not ksplit:
        knob_env("QTX_NO_SPLITK", 1)
    base = _rows_operands(gb, r, kp)
    xd = gb.init(r["res"], "xout")
    extra = {}
    if ksplit:
        part = gb.new((ksplit * M * 512,), np.int32, "part")
        extra = dict(part=part, ksplit=ksplit)
    Mp = M + (M & 1) if kp else M
    out = dict(lnq=gb.new((Mp, 512), np.int8, "lnq"), lns=gb.new((M,), f32, "lns")) if lnq \
        else dict(lnout=gb.new((M, 512), f32, "lnout"))
    rows_call(epi=1, res=xd, xout=xd, ln_a=gb.dev(la), ln_b=gb.dev(lb), **extra, **out, **base)
    gb.check()
    np.testing.assert_array_equal(np_(xd), x)
    if lnq:
        np.testing.assert_array_equal(np_(out["lns"]), s)
        if kp:
            assert_kp(np_(out["lnq"]), q, gb.poison, False, "lnq")
        else:
            np.testing.assert_array_equal(np_(out["lnq"]), q)
    else:
        np.testing.assert_array_equal(np_(out["lnout"]), ln)
    if ksplit:                    # the partials sum to the accumulators, exactly
        got = np_(part).reshape(ksplit, M, 512).astype(np.int64).sum(0)
        np.testing.assert_array_equal(got, r["acc"])


# =====================================================================================
# qtx_skinny_linear, K = 2048, N = 512, residual
# =====================================================================================
@pytest.mark.parametrize("M", [5, 40, 100, 200])
@pytest.mark.parametrize("amode", [0, 2, 3])
def test_skinny(gb, oracle_model, amode, M):
    """M = 5: the 8-wave k_skinny8_ffn2 (amode 2 / 3), whose waves reduce int32 partials
    through LDS; M = 40 / 100 / 200: k_skinny with 4- / 8- or 16- / 16-row blocks.  amode 0:
    int8 codes with random row scales; amode 2 (quantized in the prologue from complete
    partial maxima) and 3 (raw fp32): x = code * 2^-4, which quantizes back to the codes."""
    N, K = 512, 2048
    r = dict(case(M, N, K) if amode == 0 else fp32_case(M, N, K))
    r["n"] = 8 if amode == 2 else 0
    r["parts"] = None
    if amode == 2:
        r["parts"] = np.stack([np.abs(c).max(-1) for c in np.array_split(r["x"], 8, axis=1)]).astype(f32)
    rc, out, pm = _skinny_run(gb, r, amode, M, N, K, 8, RESID)
    assert_ok(rc, "qtx_skinny_linear")
    gb.check()
    y = r["res"] + O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"])
    np.testing.assert_array_equal(np_(out), y)
    gb.assert_poison(pm, "pmax_out")


# =====================================================================================
# qtx_ffn_rows, F = 2048: the fused kernel's second accumulator
# =====================================================================================
def _ffn_case(M):
    """W1 = 0 and b1 = h * 2^-4 with h the magnitudes of crafted codes: every row's hidden is
    relu(b1) = b1, which quantizes to h with the scale 2^-4.  W2 = crafted codes times the
    shared sign pattern (the hidden is non-negative, so W2 is mostly positive), odd rows
    negated: acc2[m, n] = sum_k h[k] * W2[n, k] is in [2^24, 2^25) for every n.  The rows
    share their accumulators and differ in the residual x."""
    def make():
        F_ = 2048
        lo, flip = BA.PARAMS[F_]
        rng = np.random.default_rng(BA.SEED + 100 + M)
        h = np.abs(BA.correlated_codes(rng, 1, F_, lo, flip).astype(np.int32))[0]
        w2 = BA.correlated_codes(rng, 512, F_, lo, flip).astype(np.int32) * BA.shared_signs(F_)[None, :]
        qw2 = BA.negate_half(w2.astype(np.int8))
        x1 = (rng.standard_normal((M, 512)) * 2).astype(f32)
        la = (1 + 0.1 * rng.standard_normal(512)).astype(f32)
        lb = (0.1 * rng.standard_normal(512)).astype(f32)
        qx, sx = O.quant_rows(O.layer_norm(x1, la, lb))
        qw1 = np.zeros((F_, 512), np.int8)
        sw1 = (rng.random(F_) * 0.002 + 0.0001).astype(f32)
        sw2 = (rng.random(512) * 0.002 + 0.0001).astype(f32)
        b1 = (h.astype(f32) * BA.X_SCALE).astype(f32)
        b2 = (rng.standard_normal(512) * 0.1).astype(f32)
        na = (1 + 0.1 * rng.standard_normal(512)).astype(f32)
        nb = (0.1 * rng.standard_normal(512)).astype(f32)
        hid = O.linear_epilogue(O.int_gemm(qx, qw1), sx, sw1, b1, relu=True)
        qh, sh = O.quant_rows(hid)
        assert (qh == h[None, :]).all() and (sh == BA.X_SCALE).all()
        acc2 = O.int_gemm(qh, qw2)
        st = BA.stats(acc2)
        assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24 and st["odd_big"] >= 0.40
        assert st["negative"] == 0.5
        x2 = x1 + O.linear_epilogue(acc2, sh, sw2, b2)
        ln = O.layer_norm(x2, na, nb)
        q, s = O.quant_rows(ln)
        return dict(x1=x1, qx=qx, sx=sx, qw1=qw1, sw1=sw1, qw2=qw2, sw2=sw2, b1=b1, b2=b2,
                    na=na, nb=nb, x2=x2, ln=ln, q=q, s=s)
    return memo(("ffn", M), make)


@pytest.mark.parametrize("lnq", [True, False])
@pytest.mark.parametrize("M", [7, 129])
def test_ffn_rows(gb, M, lnq):
    from qtx._lib import FfnRows
    F_ = 2048
    r = _ffn_case(M)
    wf = gb.new((F_ * 1024,), np.int8, "wf")
    call("qtx_pack_ffn", P(gb.dev(r["qw1"])), P(gb.dev(r["qw2"])), F_, P(wf), S0)
    a = FfnRows()
    a.A, a.sa, a.wf = gb.dev(to_kp(r["qx"])).data_ptr(), gb.dev(r["sx"]).data_ptr(), wf.data_ptr()
    a.sw1, a.b1 = gb.dev(r["sw1"]).data_ptr(), gb.dev(r["b1"]).data_ptr()
    a.sw2, a.b2 = gb.dev(r["sw2"]).data_ptr(), gb.dev(r["b2"]).data_ptr()
    x = gb.init(r["x1"], "x")
    a.x, a.ln_a, a.ln_b = x.data_ptr(), gb.dev(r["na"]).data_ptr(), gb.dev(r["nb"]).data_ptr()
    a.M, a.F = M, F_
    if lnq:
        q8, qs = gb.new((M + (M & 1), 512), np.int8, "lnq"), gb.new((M,), f32, "lns")
        a.lnq, a.lns = q8.data_ptr(), qs.data_ptr()
    else:
        lo = gb.new((M, 512), f32, "lnout")
        a.lnout = lo.data_ptr()
    assert_ok(lib().qtx_ffn_rows(C.byref(a), S0), "qtx_ffn_rows")
    gb.check()
    np.testing.assert_array_equal(np_(x), r["x2"])
    if lnq:
        assert_kp(np_(q8), r["q"], gb.poison, False, "lnq")
        np.testing.assert_array_equal(np_(qs), r["s"])
    else:
        np.testing.assert_array_equal(np_(lo), r["ln"])


# =====================================================================================
# qtx_linear_i8_rowfaults: a correction that carries an accumulator across 2^24
# =====================================================================================
RF_M, RF_N, RF_K = 5, 512, 2048
RF_LO, RF_FLIP = 96, 0.094      # mean |acc| near 2^24: 2048 * 111.5^2 * (1 - 2 * 0.094)^2


def _flip7(v):
    return int(np.array([v], np.int8).view(np.uint8).__xor__(np.uint8(0x80)).view(np.int8)[0])


def _crosses(before, after):
    """|acc| below 2^24 without the fault, at or above it and odd with it."""
    return (np.abs(before) < BA.TWO24) & (np.abs(after) >= BA.TWO24) & ((after & 1) == 1)


def _rowfault_case():
    def make():
        rng = np.random.default_rng(BA.SEED + 7)
        qx = BA.correlated_codes(rng, RF_M, RF_K, RF_LO, RF_FLIP)
        qw = BA.negate_half(BA.correlated_codes(rng, RF_N, RF_K, RF_LO, RF_FLIP))
        sx = (rng.random(RF_M) * 0.02 + 0.001).astype(f32)
        sw = (rng.random(RF_N) * 0.002 + 0.0001).astype(f32)
        b = rng.standard_normal(RF_N).astype(f32)
        res = rng.standard_normal((RF_M, RF_N)).astype(f32)
        acc = qx.astype(np.int64) @ qw.astype(np.int64).T
        # INPUT on row 1: the first column whose bit-7 flip carries some output across 2^24
        inp = wgt = None
        for c in range(RF_K):
            d = _flip7(qx[1, c]) - int(qx[1, c])
            hit = _crosses(acc[1], acc[1] + d * qw[:, c].astype(np.int64))
            if hit.any():
                inp = (c, int(hit.sum()))
                break
        # WEIGHT on row 3: the first (weight row, column) with the same property
        near = np.argsort(np.abs(np.abs(acc[3]) - BA.TWO24))
        for n in near[:64]:
            for c in range(RF_K):
                d = _flip7(qw[n, c]) - int(qw[n, c])
                if _crosses(acc[3, n:n + 1], acc[3, n:n + 1] + d * int(qx[3, c]))[0]:
                    wgt = (int(n), c)
                    break
            if wgt:
                break
        assert inp and wgt, "no fault found that carries an accumulator across 2^24"
        tab = {1: F("INPUT", row=0, col=inp[0], bit=7),
               3: F("WEIGHT", row=wgt[0], col=wgt[1], bit=7)}
        return qx, sx, qw, sw, b, res, tab
    return memo("rowfault", make)


def test_rowfaults_cross_2_24(gb):
    """M = 5, K = 2048: the operands put |acc| around 2^24 (both sides of it); an INPUT bit-7
    fault on row 1 and a WEIGHT bit-7 fault on row 3, found on the restatement, each carry at
    least one accumulator from below 2^24 to an odd value at or above it — the kernel's
    correction must be added in integers before the conversion, not after it."""
    from qtx import _lib
    qx, sx, qw, sw, b, res, tab = _rowfault_case()
    acc = qx.astype(np.int64) @ qw.astype(np.int64).T
    assert (np.abs(acc) < BA.TWO24).any() and (np.abs(acc) >= BA.TWO24).any()
    want = restate(qx, sx, qw, sw, b, res, RESID, tab)
    base = restate(qx, sx, qw, sw, b, res, RESID, {})
    assert (want[1] != base[1]).any() and (want[3] != base[3]).any()
    out = gb.new((RF_M, RF_N), f32, "out")
    ins = [gb.dev(a) for a in (qx, sx, qw, sw, b)]
    _lib.call("qtx_linear_i8_rowfaults", *[P(t) for t in ins], RF_M, RF_N, RF_K, RESID,
              P(gb.dev(res)), P(out), c_table(RF_M, tab), S0)
    gb.check()
    np.testing.assert_array_equal(np_(out).view(np.uint32), want.view(np.uint32))
