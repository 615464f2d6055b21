"""The integer cross-lane row maximum (wave_absmax, csrc/qtx_common.h; the bit-pattern order
alone: tests/test_absmax_bits_ref.py) in the skinny GEMM's fp32 prologues, through
qtx_skinny_linear against the oracle, bit for bit: the row maximum once in every column (so
in every lane, float4 chunk and element, and at K = 2048 in either half row of
k_skinny8_ffn2, whose waves each form the whole row's maximum), and the rows on which an
integer maximum could part from fmaxf: zeros (the 1e-5 floor), -0.0, denormals, values at the
floor, a maximum >= 2^60 (the scale's true-division path), +-inf and ties between lanes.
Random int8 weights: one wrong code or scale changes the whole output row."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ops import P, S0, _release, call, dev, torch  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 32   # two column blocks of 16


def weights(rng, K):
    return (rng.integers(-127, 128, (N, K)).astype(np.int8),
            rng.uniform(1e-3, 1e-2, N).astype(f32), rng.standard_normal(N).astype(f32))


def peak_rows(rng, K):
    """[K, K]: row i has its |x| maximum in column i alone (either sign), the rest within
    (-1, 1) of a per-row magnitude."""
    mag = rng.uniform(1e-3, 10.0, (K, 1))
    x = (rng.uniform(-1, 1, (K, K)) * mag).astype(f32)
    x[np.arange(K), np.arange(K)] = (rng.uniform(1.01, 3.0, K) * mag[:, 0] * rng.choice([-1, 1], K)).astype(f32)
    assert np.array_equal(np.abs(x).argmax(1), np.arange(K))
    return x


def special_rows(rng, K):
    base = rng.standard_normal((14, K)).astype(f32)
    x = base.copy()
    x[0] = 0.0                                               # the 1e-5 floor
    x[1] = -0.0
    den = rng.integers(1, 0x00800000, K).astype(np.uint32) | (rng.integers(0, 2, K).astype(np.uint32) << 31)
    x[2] = den.view(f32)                                     # denormals of either sign
    x[3] = x[2]
    x[3, K // 3] = np.nextafter(f32(1e-5), f32(0))           # just below the floor
    x[4] = x[2]
    x[4, K - 5] = -np.nextafter(f32(1e-5), f32(1))           # just above it
    x[5] = base[5] * f32(1e15)
    x[5, 7] = f32(2.0 ** 60)                                 # the range test's first value
    x[6] = base[6] * f32(1e17)
    x[6, K - 1] = -f32(1.5 * 2.0 ** 61)
    x[7] = base[7] * f32(1e30)
    x[7, K // 2 + 1] = f32(3e38)
    x[8, 3] = np.inf
    x[9, K - 2] = -np.inf
    x[10, 5] = np.inf
    x[10, K // 2 + 70] = -np.inf
    m = f32(4.75)                                            # ties between lanes
    x[11] = np.clip(base[11], -4, 4)
    x[11, [6, K - 9]] = m
    x[12] = np.clip(base[12], -4, 4)
    x[12, [4 * 17 + 1, K // 2 + 4 * 17 + 2]] = [m, -m]       # and across the half rows
    x[13] = np.nextafter(f32(2.0 ** 60), f32(0)) * np.sign(base[13])   # every lane just below 2^60
    return x


def run(torch, amode, x, w, M_rows, res, ln=None):
    """One call on rows M_rows of x; returns the output [M, N]."""
    qw, sw, b = w
    K = x.shape[1]
    xm = np.ascontiguousarray(x[M_rows])
    M = len(xm)
    out = dev(torch, res[M_rows].copy())
    if amode == 3:
        call("qtx_skinny_linear", 3, S0, S0, P(dev(torch, xm)), K, S0, S0, S0, 0, P(dev(torch, qw)),
             P(dev(torch, sw)), P(dev(torch, b)), M, N, K, 8, 2, P(out), P(out), S0, S0)
    else:
        call("qtx_skinny_linear", 1, S0, S0, P(dev(torch, xm)), K, P(dev(torch, ln[0])),
             P(dev(torch, ln[1])), S0, 0, P(dev(torch, qw)), P(dev(torch, sw)), P(dev(torch, b)),
             M, N, K, 8, 2, P(out), P(out), S0, S0)
    return out.cpu().numpy()


def expected(x, w, res, ln=None):
    qw, sw, b = w
    with np.errstate(all="ignore"):
        qx, sx = O.quant_rows(x if ln is None else O.layer_norm(x, *ln))
        return res + O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b)


@pytest.mark.parametrize("K,MB", [(512, 64), (2048, 32)])
def test_row_maximum_in_every_column(torch, K, MB):
    """amode 3.  K = 512: k_skinny's own-row prologue, 64 rows per call.  K = 2048 with the
    residual epilogue at M = 32: k_skinny8_ffn2 — the maximum in every column of either half."""
    rng = np.random.default_rng(K)
    x, w = peak_rows(rng, K), weights(rng, K)
    res = rng.standard_normal((K, N)).astype(f32)
    want = expected(x, w, res)
    for m0 in range(0, K, MB):
        rows = np.arange(m0, m0 + MB)
        np.testing.assert_array_equal(run(torch, 3, x, w, rows, res), want[rows], err_msg=f"rows {m0}..")


@pytest.mark.parametrize("K", [512, 2048])
def test_special_rows(torch, K):
    """Zeros, -0.0, denormals, the floor's neighbours, maxima >= 2^60, +-inf, ties — all rows
    in one call (K = 2048: 14 rows, k_skinny8_ffn2) and in calls of M = 1, 3, 4, 5."""
    rng = np.random.default_rng(K + 1)
    x, w = special_rows(rng, K), weights(rng, K)
    res = rng.standard_normal((len(x), N)).astype(f32)
    want = expected(x, w, res)
    np.testing.assert_array_equal(run(torch, 3, x, w, np.arange(len(x)), res), want)
    off = 0
    for M in (1, 3, 4, 5, 1, 3, 4, 5):                      # 26 rows: every special row at least once
        rows = (off + np.arange(M)) % len(x)
        np.testing.assert_array_equal(run(torch, 3, x, w, rows, res), want[rows], err_msg=f"M {M} from {off}")
        off += M


@pytest.mark.parametrize("M", [1, 3, 4, 5])
def test_small_m_peaks(torch, M):
    """The peak rows again in blocks that leave rows of the 4-row workgroup empty."""
    for K in (512, 2048):
        rng = np.random.default_rng(K)                      # the arrays of the test above
        x, w = peak_rows(rng, K), weights(rng, K)
        res = rng.standard_normal((K, N)).astype(f32)
        rows = (np.arange(M) * 131 + 17 * M) % K
        np.testing.assert_array_equal(run(torch, 3, x, w, rows, res), expected(x[rows], w, res[rows]))


def test_layernorm_outlier_in_every_column(torch):
    """amode 1 (LayerNorm prologue, quant_rows512): an outlier in column i of row i, so the
    normalized row's maximum sits there; 64 rows per call."""
    K = 512
    rng = np.random.default_rng(3)
    x = rng.standard_normal((K, K)).astype(f32)
    x[np.arange(K), np.arange(K)] += (rng.choice([-1, 1], K) * rng.uniform(8, 20, K)).astype(f32)
    ln = (rng.uniform(0.9, 1.1, K).astype(f32), (0.1 * rng.standard_normal(K)).astype(f32))
    w = weights(rng, K)
    res = rng.standard_normal((K, N)).astype(f32)
    want = expected(x, w, res, ln)
    assert np.array_equal(np.abs(O.layer_norm(x, *ln)).argmax(1), np.arange(K))
    for m0 in range(0, K, 64):
        rows = np.arange(m0, m0 + 64)
        np.testing.assert_array_equal(run(torch, 1, x, w, rows, res, ln), want[rows], err_msg=f"rows {m0}..")
