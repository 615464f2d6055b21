"""The fragment mapping of k_dec_attn's scores (csrc/qtx_decode.hip) as a numpy model: the
key rows are loaded straight into the B-operand layout of the int8 16x16x64 MFMA, the q
codes fill every row of A, and each lane picks its keys' dot products out of C.

The operands are built per lane exactly as the kernel indexes them; the MFMA is the layout
k_skinny relies on (A and B: row / column lane & 15, byte chunk lane >> 4; C: column
lane & 15, row 4 (lane >> 4) + e)."""
import numpy as np
import pytest

LANES = np.arange(64)
FR, FG = LANES & 15, LANES >> 4


def mfma_i32_16x16x64_i8(a_op, b_op):
    """a_op, b_op [64 lanes, 16 bytes] int8 -> the lanes' four int32 results [64, 4]."""
    A = np.zeros((16, 64), np.int64)
    Bm = np.zeros((64, 16), np.int64)
    for l in LANES:
        A[FR[l], 16 * FG[l]:16 * FG[l] + 16] = a_op[l]
        Bm[16 * FG[l]:16 * FG[l] + 16, FR[l]] = b_op[l]
    Cm = A @ Bm
    out = np.zeros((64, 4), np.int64)
    for l in LANES:
        for e in range(4):
            out[l, e] = Cm[4 * FG[l] + e, FR[l]]
    return out


def kernel_scores(q, kcache, nrows, step=None, knew=None):
    """The kernel's per-lane scores [64 lanes, slots]: kcache [>= nrows, 64] int8 is the
    head's cached key rows; (self) knew [64] replaces row `step` in registers."""
    nit = (nrows + 15) // 16
    qs = q.copy()                                       # LDS row of the q codes
    qf = np.stack([qs[16 * FG[l]:16 * FG[l] + 16] for l in LANES])
    kr = []
    for i in range(nit):
        rows = np.minimum(16 * i + FR, nrows - 1)       # clamped: duplicates of the last row
        kr.append(np.stack([kcache[rows[l], 16 * FG[l]:16 * FG[l] + 16] for l in LANES]))
    if step is not None:
        kn = np.stack([knew[16 * FG[l]:16 * FG[l] + 16] for l in LANES])
        for i in range(nit):                            # unrolled compare-and-select
            sel = (i == (step >> 4)) & (FR == (step & 15))
            kr[i] = np.where(sel[:, None], kn, kr[i])
    acc = [mfma_i32_16x16x64_i8(qf, kr[i]) for i in range(nit)]
    nu = 2 if nit > 4 else 1
    dot = np.zeros((64, nu), np.int64)
    for u in range(nu):
        for l in LANES:
            d = acc[4 * u][l, 0]
            for t in range(1, 4):
                if 4 * u + t < nit and FG[l] == t:
                    d = acc[4 * u + t][l, 0]
            dot[l, u] = d
    return dot, acc


def check(dot, acc, q, keys, n):
    """Keys 0 .. n - 1: lane j % 64, slot j / 64 holds q . k_j; every C row holds the same."""
    want = keys[:n].astype(np.int64) @ q.astype(np.int64)
    for j in range(n):
        assert dot[j & 63, j >> 6] == want[j], j
    for i, c in enumerate(acc):
        for e in range(1, 4):
            np.testing.assert_array_equal(c[:, e], c[:, 0])
        for l in LANES:                                  # column fr of fragment i is key 16 i + fr
            j = 16 * i + FR[l]
            if j < n:
                assert c[l, 0] == want[j]


@pytest.mark.parametrize("nrows", [1, 15, 16, 17, 63, 64, 65, 72, 127, 128])
def test_cross_rows(nrows):
    rng = np.random.default_rng(nrows)
    q = rng.integers(-127, 128, 64).astype(np.int8)
    keys = rng.integers(-127, 128, (nrows, 64)).astype(np.int8)
    dot, acc = kernel_scores(q, keys, nrows)
    check(dot, acc, q, keys, nrows)
    # the clamped lanes hold duplicates of the last row, never another key's
    last = int(keys[nrows - 1].astype(np.int64) @ q.astype(np.int64))
    nit = (nrows + 15) // 16
    for l in LANES:
        if 16 * (nit - 1) + FR[l] >= nrows:
            assert acc[nit - 1][l, 0] == last


@pytest.mark.parametrize("host_pos", [False, True])
@pytest.mark.parametrize("step", [0, 1, 15, 16, 31, 47, 48, 63, 64, 65, 79, 80, 127])
def test_self_new_key_patch(step, host_pos):
    """Row `step` of the cache is stale; the new k codes replace it in registers.  With the
    position from the host step + 1 rows are loaded, else all 128 allocated."""
    rng = np.random.default_rng(1000 + step)
    q = rng.integers(-127, 128, 64).astype(np.int8)
    cache = rng.integers(-127, 128, (128, 64)).astype(np.int8)
    knew = rng.integers(-127, 128, 64).astype(np.int8)
    nrows = step + 1 if host_pos else 128
    dot, acc = kernel_scores(q, cache, nrows, step, knew)
    keys = cache.copy()
    keys[step] = knew
    assert not np.array_equal(cache[step], knew)
    check(dot, acc, q, keys, step + 1)
    if not host_pos:                                     # rows past the position: untouched
        check(dot, acc, q, keys, 128)


def test_extremes():
    """|acc| = 64 * 127^2 fits int32 and comes out in the key's own lane."""
    q = np.full(64, 127, np.int8)
    keys = np.zeros((72, 64), np.int8)
    for j in range(72):
        k = keys.copy()
        k[j] = -127 if j & 1 else 127
        dot, _ = kernel_scores(q, k, 72)
        want = np.zeros(72, np.int64)
        want[j] = (-1 if j & 1 else 1) * 64 * 127 * 127
        got = np.array([dot[i & 63, i >> 6] for i in range(72)])     # keys 0 .. 71
        np.testing.assert_array_equal(got, want)
