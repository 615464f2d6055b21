"""wave_absmax (csrc/qtx_common.h) restated in numpy, no GPU: for lane values that are >= +0
and not NaN, the unsigned-integer maximum of the bit patterns over the DPP tree equals the
fmaxf tree's result (wave_max), bit for bit — the order of such floats is the order of their
bit patterns.  Both trees are evaluated level by level as the kernels do (xor 1, xor 2,
half-mirror, mirror inside each 16-lane row, then the four rows' lane 0 / 16 / 32 / 48)."""
import numpy as np
import pytest

f32, u32 = np.float32, np.uint32
INF_BITS = 0x7F800000
LANES = np.arange(64)
# source lane of each DPP level: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
# (lane 7 - i of its 8), row_mirror (lane 15 - i of its 16)
LEVELS = (LANES ^ 1, LANES ^ 2, (LANES & ~7) | (7 - (LANES & 7)), (LANES & ~15) | (15 - (LANES & 15)))


def tree(v, op):
    """[..., 64] lane values -> [...] wave result of the kernels' reduction with `op`."""
    for src in LEVELS:
        v = op(v, v[..., src])
    return op(op(v[..., 0], v[..., 16]), op(v[..., 32], v[..., 48]))


def check(bits, floor=f32(0.0)):
    bits = np.asarray(bits, u32)
    assert bits.max() <= INF_BITS            # the precondition: >= +0, not NaN
    x = bits.view(f32)
    want = np.fmax(tree(x, np.fmax), floor)                  # fmaxf(wave_max(x), floor)
    got = np.maximum(tree(bits, np.maximum), np.asarray(floor, f32).view(u32))
    np.testing.assert_array_equal(got, want.view(u32))
    np.testing.assert_array_equal(got, np.maximum(bits.max(-1), np.asarray(floor, f32).view(u32)))


@pytest.mark.parametrize("floor", [0.0, 1e-5])
def test_random_patterns(floor):
    rng = np.random.default_rng(10)
    check(rng.integers(0, INF_BITS + 1, (4096, 64), dtype=np.int64).astype(u32), f32(floor))
    # values around the floor and around 2^60 (the scale's range test)
    for centre in (f32(1e-5).view(u32), f32(2.0 ** 60).view(u32)):
        check((int(centre) + rng.integers(-40, 41, (512, 64))).astype(u32), f32(floor))


@pytest.mark.parametrize("floor", [0.0, 1e-5])
def test_denormals_zero_inf(floor):
    rng = np.random.default_rng(11)
    den = rng.integers(0, 0x00800000, (512, 64)).astype(u32)       # +0 and denormals only
    check(den, f32(floor))
    check(np.zeros((1, 64), u32), f32(floor))                      # all +0: the floor alone
    mixed = rng.integers(0, INF_BITS + 1, (256, 64), dtype=np.int64).astype(u32)
    mixed[np.arange(256), rng.integers(0, 64, 256)] = INF_BITS     # +inf in one lane
    check(mixed, f32(floor))
    check(np.full((1, 64), INF_BITS, u32), f32(floor))


def test_maximum_in_each_lane_and_ties():
    rng = np.random.default_rng(12)
    base = rng.integers(0, 0x3F800000, (64, 64)).astype(u32)       # < 1.0
    for top in (f32(1.0).view(u32), u32(1), u32(INF_BITS), f32(2.0 ** 60).view(u32)):
        b = np.minimum(base, u32(max(int(top) - 1, 0)))
        b[LANES, LANES] = top                                      # row l: the maximum in lane l
        check(b)
        check(b, f32(1e-5))
        t = b.copy()
        t[LANES, (LANES * 7 + 3) % 64] = top                       # a second lane ties with it
        check(t)
        check(t, f32(1e-5))


def test_precondition_is_needed():
    """Negative values (and -0.0) order the other way as integers: the lane-local stage must
    hand over |x| maxima from +0 (fmaxf(0, |x| ...)), which the kernels do."""
    x = np.full(64, 0.5, f32)
    x[5], x[9] = -1.0, -0.0
    assert tree(x.view(u32), np.maximum) == f32(-1.0).view(u32)    # not the float maximum, 0.5
    assert tree(x, np.fmax) == f32(0.5)
    lane_local = np.fmax(f32(0.0), np.abs(x))                      # what reaches wave_absmax
    assert lane_local.view(u32)[9] == 0
    check(lane_local.view(u32)[None])
