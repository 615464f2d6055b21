"""The conditions the inputs of tests/test_gpu_big_acc.py must meet, checked on the oracle
alone (tests/big_acc.py builds them): the accumulators sit in [2^24, 2^25), where the fp32
spacing is 2 and every odd accumulator is an exact tie of float(acc); enough of them are odd,
half are negative, and the oracle's round-to-nearest-even differs from truncation and from
round-half-away on enough of the odd ones that a kernel converting either way fails the
bit-for-bit comparison.  The control: random codes, as every other test draws them, stay far
below 2^24."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_acc as BA  # noqa: E402

f32 = np.float32


def _acc(M, N, K):
    lo, flip = BA.PARAMS[K]
    qx, qw = BA.operands(BA.SEED, M, N, K, lo, flip)
    return qx, qw, O.int_gemm(qx, qw)


def test_codes_are_as_described():
    rng = np.random.default_rng(3)
    q = BA.correlated_codes(rng, 37, 2048, 96, 0.02)
    assert q.dtype == np.int8 and q.shape == (37, 2048)
    mag = np.abs(q.astype(np.int32))
    assert mag.min() >= 96 and mag.max() == 127 and (mag.max(axis=1) == 127).all()
    # magnitudes uniform over [96, 127]: every value occurs, the mean is near 111.5
    assert set(np.unique(mag)) == set(range(96, 128)) and abs(mag.mean() - 111.5) < 0.5
    disagree = (np.sign(q) != BA.shared_signs(2048)[None, :]).mean()
    assert 0.01 < disagree < 0.03                       # flip = 0.02
    assert abs((BA.shared_signs(2048) > 0).mean() - 0.5) < 0.05
    w = BA.negate_half(q)
    np.testing.assert_array_equal(w[0::2], q[0::2])
    np.testing.assert_array_equal(w[1::2], -q[1::2])


def test_fp32_form_quantizes_back_exactly():
    """x = code * 2^-4: the per-token quantizer returns the crafted codes and the scale 2^-4."""
    qx, _, _ = _acc(37, 64, 2048)
    x = BA.as_fp32(qx)
    q, s = O.quant_rows(x)
    np.testing.assert_array_equal(q, qx)
    np.testing.assert_array_equal(s, np.full(37, 2.0 ** -4, f32))


def test_rounding_alternatives_are_what_they_say():
    a = np.array([(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, -(1 << 24) - 3, 5, (1 << 24) + 2,
                  (1 << 25) + 2, (1 << 25) + 6, -(1 << 25) - 3])
    rne = a.astype(np.int32).astype(f32).astype(np.int64) - a
    np.testing.assert_array_equal(rne, [-1, 1, 1, -1, 0, 0, -2, 2, -1])
    np.testing.assert_array_equal(BA.to_float_trunc(a).astype(np.int64) - a,
                                  [-1, -1, 1, 1, 0, 0, -2, -2, 3])
    np.testing.assert_array_equal(BA.to_float_half_away(a).astype(np.int64) - a,
                                  [1, 1, -1, -1, 0, 0, 2, 2, -1])


def test_k2048_accumulators_are_ties():
    """K = 2048, lo = 96, flip = 0.02, M x N = 37 x 64, seed 1.  Measured: |acc| in
    [22,777,416, 24,325,719]; 48.3 % odd; exactly half negative; astype(float32) differs from
    truncation on 50.2 % and from round-half-away on 49.8 % of the odd ones."""
    _, _, acc = _acc(37, 64, 2048)
    st = BA.stats(acc)
    assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24
    assert st["odd_big"] >= 0.40
    assert st["negative"] == 0.5
    assert (acc[:, 0::2] > 0).all() and (acc[:, 1::2] < 0).all()
    assert st["vs_trunc"] >= 0.40 and st["vs_half_away"] >= 0.40


def test_k1280_accumulators_are_ties():
    """K = 1280 (the smallest model K above 1041; at M = 37 the 32-tile k_gemm), lo = 120,
    flip = 0.01, M x N = 37 x 64, seed 1.
    Measured: |acc| in [18,287,852, 19,193,554], all >= 2^24; 49.6 % odd (the issue asks for
    at least 25 % odd with |acc| >= 2^24); half negative; astype(float32) differs from
    truncation on 48.3 % and from round-half-away on 51.7 % of the odd ones."""
    _, _, acc = _acc(37, 64, 1280)
    st = BA.stats(acc)
    assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24
    assert st["odd_big"] >= 0.25
    assert st["negative"] == 0.5
    assert st["vs_trunc"] >= 0.40 and st["vs_half_away"] >= 0.40


def test_k1344_accumulators_are_ties():
    """K = 1344 (not a multiple of 256: with M >= 256 the 128-tile k_gemm), lo = 120,
    flip = 0.01, 257 x 272: all |acc| in [2^24, 2^25), at least 40 % odd."""
    _, _, acc = _acc(257, 272, 1344)
    st = BA.stats(acc)
    assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24
    assert st["odd_big"] >= 0.40 and st["negative"] == 0.5
    assert st["vs_trunc"] >= 0.40 and st["vs_half_away"] >= 0.40


@pytest.mark.parametrize("M,N", [(257, 272), (5, 512), (40, 512), (100, 512), (200, 512),
                                 (7, 512), (129, 512)])
def test_every_gpu_shape_is_in_range(M, N):
    """The other K = 2048 shapes of test_gpu_big_acc.py: all in [2^24, 2^25), >= 40 % odd."""
    _, _, acc = _acc(M, N, 2048)
    st = BA.stats(acc)
    assert BA.TWO24 <= st["min_abs"] and st["max_abs"] < 2 * BA.TWO24 and st["odd_big"] >= 0.40
    assert st["vs_trunc"] >= 0.40 and st["vs_half_away"] >= 0.40


def test_control_random_codes_stay_below_2_24():
    """Why no older test reaches the regime: uniform random codes at K = 2048 give a largest
    |acc| over 37 x 64 outputs of about 9e5 (918,614 with this seed), 18 times below 2^24 —
    where float(acc) is exact and every rounding mode agrees."""
    rng = np.random.default_rng(0)
    acc = O.int_gemm(rng.integers(-127, 128, (37, 2048)), rng.integers(-127, 128, (64, 2048)))
    assert np.abs(acc).max() < BA.TWO24 // 8
    a = acc.astype(np.int64)
    np.testing.assert_array_equal(BA.to_float_trunc(a), a.astype(f32))
    np.testing.assert_array_equal(BA.to_float_half_away(a), a.astype(f32))


def test_int4_weights_cannot_reach_2_24():
    assert 7 * 127 * 2048 < BA.TWO24
