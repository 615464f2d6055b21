"""Rounding-edge inputs for the per-token quantizers (helper, no GPU).

Every quantizer of the library computes q = rint(x / s) with some shortcut for the quotient
(x * v_rcp_f32(s) behind a near-tie vote, Markstein's div_cr, the hardware's ties-to-even in
the code packing).  Gaussian rows almost never land where the shortcut and the true quotient
part ways: on a rounding tie x / s == k + 1/2 and its floating-point neighbours.  tie_rows()
builds rows that consist of those points; the model_*() functions restate the ways a
quantizer can be wrong, and discrimination() counts, for any fp32 rows a site quantizes, how
many codes each wrong model gets wrong against the oracle.  tests/test_rounding_edges_ref.py
asserts those counts on the CPU; tests/test_gpu_rounding_edges.py feeds the same arrays to
the kernels."""
import functools
from fractions import Fraction

import numpy as np

from oracle import qtx_oracle as O

f32 = np.float32
# odd mantissas < 256 of the scale.  5, 9 and 17 separate nothing (model (a) gets every code
# right); 3 separates too little (36 of 1271 codes, below the per-set bound of the CPU test)
# and is replaced by 125.  With qmax 7 the mantissa 7 is the weak one (7 * s has mantissa 49).
MANTS = (7, 15, 61, 63, 255, 125)
MANTS_Q7 = (15, 61, 63, 255, 125, 41)
EXPS = (-12, -3, 5)
COMBOS = tuple((m, e) for e in EXPS for m in MANTS)      # neighbours differ in mantissa
COMBOS_Q7 = tuple((m, e) for e in EXPS for m in MANTS_Q7)
SEED = 20250117


def scale_of(mant, exp):
    assert mant % 2 == 1 and 0 < mant < 256
    return f32(np.ldexp(float(mant), exp))


def _exact32(v):
    """float64 values that must be float32 values already."""
    w = np.asarray(v, np.float64).astype(f32)
    assert np.array_equal(w.astype(np.float64), v), "not exact in float32"
    return w


def tie_pattern(mant, exp, qmax=127.0):
    """(values f32 [n, 5], k int [n]): row i holds the tie s * (k_i + 1/2), then its
    nextafter once and twice upwards, once and twice downwards, for every k with
    |k + 1/2| < qmax."""
    s = float(scale_of(mant, exp))
    k = np.arange(-int(qmax), int(qmax))
    t = _exact32(s * (k + 0.5))
    up, dn = f32(np.inf), f32(-np.inf)
    u1, d1 = np.nextafter(t, up), np.nextafter(t, dn)
    return np.stack([t, u1, np.nextafter(u1, up), d1, np.nextafter(d1, dn)], 1), k


@functools.lru_cache(maxsize=None)
def _tie_rows(D, mant, exp, qmax):
    s = scale_of(mant, exp)
    top = _exact32(float(qmax) * float(s))
    assert f32(top / f32(qmax)) == s            # the row's scale is exactly s
    pat, k = tie_pattern(mant, exp, qmax)
    n = len(k)
    iq = int(qmax)
    ints = _exact32(float(s) * np.array([1, -2, iq // 2, -(iq - 1)], np.float64))
    extras = np.concatenate([[top], ints, [f32(0), f32(0)]]).astype(f32)
    cap = D - len(extras)
    R = -(-max(pat.size, 1270) // cap)      # a small pattern (qmax 7) still fills as many rows
    # tie i (sorted by k, so i // 2 keeps an even and an odd k together) and variant v go to
    # row (i // 2 + v) % R: every row gets ties of both parities and every variant
    rows = [[] for _ in range(R)]
    for v in range(5):
        for i in range(n):
            rows[(i // 2 + v) % R].append((i, v))
    flat = [(i, v) for v in range(5) for i in range(n)]
    rng = np.random.default_rng(SEED + D + mant)
    out = np.empty((R, D), f32)
    for r, own in enumerate(rows):
        assert len(own) <= cap
        j = (r * 131) % len(flat)
        while len(own) < cap:                   # fill up with the pattern again
            own.append(flat[j])
            j = (j + 1) % len(flat)
        vals = np.concatenate([extras, [pat[i, v] for i, v in own]]).astype(f32)
        is_tie = np.concatenate([np.zeros(len(extras), bool), [v == 0 for _, v in own]])
        p = rng.permutation(D)
        vals, is_tie = vals[p], is_tie[p]
        edge = list(range(4)) + list(range(D - 4, D))
        spare = [c for c in np.flatnonzero(is_tie) if c not in edge]
        for c in edge:                          # the first and last float4 hold ties
            if not is_tie[c]:
                d = spare.pop()
                vals[[c, d]] = vals[[d, c]]
                is_tie[[c, d]] = is_tie[[d, c]]
        assert is_tie[edge].all()
        out[r] = vals
    out.setflags(write=False)
    return out


def tie_rows(D, mant, exp, qmax=127.0):
    """float32 rows [R, D] (read-only, cached) whose per-row scale max|x| / qmax is exactly
    s = mant * 2**exp and whose other elements are the rounding ties s * (k + 1/2) of every k
    with |k + 1/2| < qmax, their neighbours one and two ulps to either side, a few exact
    integers s * k and zeros, at positions permuted with a fixed seed.  R is what the pattern
    needs at width D; short rows are filled with the pattern again."""
    return _tie_rows(int(D), int(mant), int(exp), float(qmax))


def tie_mask(x, s):
    """Elements with x / s == k + 1/2 exactly (rational arithmetic)."""
    fs = Fraction(float(s))
    flat = [(Fraction(float(v)) / fs * 2) for v in np.asarray(x).reshape(-1)]
    m = np.array([q.denominator == 1 and q.numerator % 2 == 1 for q in flat])
    return m.reshape(np.shape(x))


# ------------------------------------------------------------------ wrong quantizers
def _codes(q, relu):
    q = np.asarray(q, np.float64)
    return np.maximum(q, 0) if relu else q


def model_recip(x, s, ulps=0, relu=False):
    """(a) / (b): rint(fl(x * y)) with y = RN(1 / s) moved by `ulps` float32 steps — the
    near-tie fallback removed, or div_cr without its correction (q = a * y only)."""
    s = np.asarray(s, f32)[..., None]
    y = (f32(1.0) / s).astype(f32)
    for _ in range(abs(ulps)):
        y = np.nextafter(y, f32(np.inf) if ulps > 0 else f32(0))
    return _codes(np.rint((np.asarray(x, f32) * y).astype(f32)), relu)


def model_half_away(x, s, relu=False):
    """(c): the correctly rounded quotient rounded half away from zero."""
    q = (np.asarray(x, f32) / np.asarray(s, f32)[..., None]).astype(np.float64)
    return _codes(np.sign(q) * np.floor(np.abs(q) + 0.5), relu)


def discrimination(x, n_bits=8, relu=False):
    """For fp32 rows x [R, D] that a site quantizes per row: the oracle's (codes, scales), and
    per row the number of codes each wrong model gets wrong, as a dict of int arrays [R] with
    keys 'a', 'b_lo', 'b_hi', 'c'.  relu: the site quantizes max(x, 0) and packs the code of
    x clamped at 0."""
    x = np.asarray(x, f32)
    xr = np.where(x > 0, x, f32(0)).astype(f32) if relu else x
    q, s = O.quant_rows(xr, n_bits)
    ref = q.astype(np.float64)
    cnt = dict(a=(model_recip(x, s, 0, relu) != ref).sum(-1),
               b_lo=(model_recip(x, s, -1, relu) != ref).sum(-1),
               b_hi=(model_recip(x, s, +1, relu) != ref).sum(-1),
               c=(model_half_away(x, s, relu) != ref).sum(-1))
    return (q, s), cnt


# ------------------------------------------------------------------ one near-tie per row
# In a tie row every lane of every wave holds a near-tie, so a wave-wide vote always takes the
# true division: such rows cannot tell whether the vote sees each of a lane's values, or how
# wide its window is.  A lone row holds exactly ONE element near a tie — one that a wrong model
# gets wrong, and among those the one whose reciprocal product lies farthest from the tie —
# and otherwise exact integers s * k, whose quotients no model moves.
LONE_MODELS = (("a", 0), ("b_lo", -1), ("b_hi", +1))


@functools.lru_cache(maxsize=None)
def lone_rows(D):
    """(rows f32 [3 * D/64, D], cols int, models): row 3 * slot + t holds its lone near-tie at
    column 256 * (slot // 4) + 4 * lane + slot % 4 — slot runs over the D/64 positions a lane
    can hold the value in (float4 chunk lane + 64 j, element e), the lane varies from row to
    row — and it is one that model LONE_MODELS[t] gets wrong.  The (mantissa, exponent) sets
    are taken in turn; the lone element is positive, so a ReLU site keeps it."""
    n = 3 * (D // 64)
    out = np.empty((n, D), f32)
    cols = np.empty(n, np.int64)
    for idx in range(n):
        slot, t = divmod(idx, 3)
        mant, exp = COMBOS[idx % len(COMBOS)]
        s = scale_of(mant, exp)
        lane = (11 * idx + 5) % 64
        col = 256 * (slot // 4) + 4 * lane + slot % 4
        k = (np.arange(D) * 37 + idx) % 253 - 126
        row = _exact32(float(s) * k.astype(np.float64))
        row[(col + 130) % D] = f32(127.0) * s
        pat, kk = tie_pattern(mant, exp)
        cand = pat[kk >= 0].reshape(-1)
        ref = np.rint(cand / s)
        wrong = model_recip(cand[None], np.array([s]), LONE_MODELS[t][1])[0] != ref
        assert wrong.any()
        y = f32(1.0) / s
        for _ in range(abs(LONE_MODELS[t][1])):
            y = np.nextafter(y, f32(np.inf) if LONE_MODELS[t][1] > 0 else f32(0))
        r = (cand * y).astype(f32).astype(np.float64)
        dist = np.where(wrong, np.abs(r - np.floor(r) - 0.5), -1.0)
        row[col] = cand[np.argmax(dist)]
        out[idx], cols[idx] = row, col
    return _ro(out), _ro(cols), tuple(m for _ in range(D // 64) for m, _ in LONE_MODELS)


# ------------------------------------------------------------------ constructions
# Each builder returns the arrays one GPU case feeds to a kernel; the expected results are
# the oracle's on exactly those arrays.  The case lists are shared too, so the CPU test counts
# on the very rows the GPU test sends.
# (amode, K, pmax_n, M, start) of the skinny prologue cases that take the rows as they are
SKINNY_DIRECT = tuple((amode, K, nparts, M, (M + K // 512 + nparts) % len(COMBOS))
                      for amode, K, nparts in ((3, 512, 0), (3, 2048, 0), (2, 512, 8),
                                               (2, 2048, 128), (2, 2048, 32))
                      for M in (3, 40, 100))
# (start, kind) of each call of a GEMM-epilogue case (onehot_gemm)
ONEHOT_QKV = (tuple((s, "ties") for s in (0, 3, 6, 9, 12, 15))
              + ((2, "lone"), (13, "lone"), (4, "bias"), (11, "bias")))
ONEHOT_FFN1 = (tuple((s, "ties") for s in (0, 7, 14, 3, 10, 17))
               + ((5, "lone"), (40, "lone"), (2, "bias"), (15, "bias")))
FFN_HIDDEN_STARTS = (1, 8, 15, 4, 11, 12)
DECODE_CROSS_Q = (512, 4, 9)                   # direct_rows arguments of the cross attention's q


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def all_rows(D, qmax=127.0):
    """Every row of every (mantissa, exponent) set at width D."""
    combos = COMBOS if qmax == 127.0 else COMBOS_Q7
    return _ro(np.concatenate([tie_rows(D, m, e, qmax) for m, e in combos]))


@functools.lru_cache(maxsize=None)
def combo_rows(D, n, start=0, lone=False):
    """n rows of width D: row i comes from set COMBOS[(start + i) % 18], and within the set
    the rows are taken in turn.  lone: n rows of lone_rows(D) from row `start` on instead."""
    out = np.empty((n, D), f32)
    if lone:
        rows = lone_rows(D)[0]
        return _ro(rows[(start + np.arange(n)) % len(rows)])
    for i in range(n):
        m, e = COMBOS[(start + i) % len(COMBOS)]
        r = tie_rows(D, m, e)
        out[i] = r[((start + i) // len(COMBOS)) % len(r)]
    return _ro(out)


@functools.lru_cache(maxsize=None)
def betas():
    """The LayerNorm beta vectors [18 + 24, 512]: one tie row of each (mantissa, exponent) set
    (the three rows of the 512-wide pattern in turn), then the 24 lone rows."""
    return _ro(np.concatenate([combo_rows(512, len(COMBOS), 0), lone_rows(512)[0]]))


N_TIE_BETAS = len(COMBOS)


@functools.lru_cache(maxsize=None)
def direct_rows(K, M, start):
    """(rows [M, K], lone [M] bool) of a direct-input case: tie rows at the even positions,
    lone rows at the odd ones."""
    out = np.empty((M, K), f32)
    out[0::2] = combo_rows(K, (M + 1) // 2, start)
    out[1::2] = combo_rows(K, M // 2, start, lone=True)
    return _ro(out), _ro(np.arange(M) % 2 == 1)


def mostly_positive(row):
    """A ReLU site keeps only the positive half of a tie row; on a narrow row that leaves too
    few ties, so the negative elements are mirrored except in one column of 8 (those still go
    through the clamp to code 0)."""
    keep = (np.arange(row.shape[-1]) % 8) == 5
    return _ro(np.where((row < 0) & ~keep, -row, row).astype(f32))


@functools.lru_cache(maxsize=None)
def ffn_hidden_bias(F, start):
    """b1 of the fused FFN's hidden quantizer (A = 0, so h = relu(b1)): the F-wide tie row of
    set `start`; at F = 256 mostly positive."""
    row = combo_rows(F, 1, start)[0]
    return mostly_positive(row) if F < 2048 else row


@functools.lru_cache(maxsize=None)
def decode_y(B, start=4, lone=False):
    """The decode step's q | k | v projections [B, 1536]: three 512-wide tie rows (or lone
    rows) of three different sets per sentence."""
    return _ro(combo_rows(512, 3 * B, start, lone).reshape(B, 1536))


def rand_weights(rng, N, K):
    """Random int8 codes, scales and bias of a linear (one wrong input code changes the
    whole output row)."""
    return (rng.integers(-127, 128, (N, K)).astype(np.int8),
            rng.uniform(1e-3, 1e-2, N).astype(f32), rng.standard_normal(N).astype(f32))


@functools.lru_cache(maxsize=None)
def onehot_gemm(M, N, start, kind="ties"):
    """A GEMM whose output rows are tie rows with a different power-of-two factor per row:
    A[m, 0] = 1, W[n, 0] = 1 (every other code 0), sa[m] = 2**(m % 5 - 2), bias 0 and sw = tie
    rows (one 512-wide row of a different set per 512-column tile, or one 2048-wide row; kind
    "lone": lone rows), so y[m, n] = (1 * sa[m]) * sw[n] + 0 with every product exact.
    kind "bias": the rows go in as the bias and sw = 0, so y[m, :] = 0 + b: the tie row as it
    is, through the epilogue's addition."""
    lone = kind == "lone"
    qx = np.zeros((M, 512), np.int8)
    qx[:, 0] = 1
    qw = np.zeros((N, 512), np.int8)
    qw[:, 0] = 1
    sa = np.ldexp(f32(1), (np.arange(M) % 5) - 2).astype(f32)
    if N == 2048:
        sw = combo_rows(2048, 1, start, lone)[0]
    else:
        sw = combo_rows(512, N // 512, start, lone).reshape(-1)
    b = np.zeros(N, f32)
    if kind == "bias":
        sw, b = b, sw
    return dict(qx=_ro(qx), qw=_ro(qw), sa=_ro(sa), sw=_ro(sw), b=_ro(b))


@functools.lru_cache(maxsize=None)
def encq_case(B, S, seed=0):
    """Encoder attention whose context is a near-tie row: each sentence keeps exactly one key
    (a different one per sentence), so P = 127/127 there and the context of every query is
    float(v) * s_v of that key; v in {-1, 0, 1} with one 2 per token, so the scale is
    RN(2 s_v / 127) and the quotients are +-63.5 (1 +- a few ulps)."""
    rng = np.random.default_rng(1000 * seed + 11 * S + B)
    q, k = (rng.integers(-127, 128, (B, S, 512)).astype(np.int8) for _ in range(2))
    v = rng.integers(-1, 2, (B, S, 512)).astype(np.int8)
    pos = rng.integers(0, 512, (B, S))
    np.put_along_axis(v, pos[..., None], 2, axis=-1)
    sq, sk, sv = (rng.uniform(0.002, 0.03, (B, S)).astype(f32) for _ in range(3))
    km = np.zeros((B, S), np.uint8)
    keep = (np.arange(B) * 5 + 3) % S
    km[np.arange(B), keep] = 1
    for b in range(B):
        # whether fl(x * RN(1/s)) falls on the other side of 63.5 than fl(x / s) depends on
        # s_v's mantissa (about one draw in eight): redraw the kept key's scale until it does
        while discrimination(v[b, keep[b]].astype(f32)[None] * sv[b, keep[b]])[1]["a"][0] < 8:
            sv[b, keep[b]] = f32(rng.uniform(0.002, 0.03))
    return dict(q=_ro(q), k=_ro(k), v=_ro(v), sq=_ro(sq), sk=_ro(sk), sv=_ro(sv), km=_ro(km),
                keep=_ro(keep))


@functools.lru_cache(maxsize=None)
def encq_expected(B, S, seed=0):
    """The oracle's (context fp32 [B, S, 512], codes, scales) of encq_case."""
    c = encq_case(B, S, seed)
    ctx, _ = O.attention(c["q"], c["sq"], c["k"], c["sk"], c["v"], c["sv"], c["km"][:, None, :], 8)
    qc, sc = O.quant_rows(ctx)
    return _ro(ctx), _ro(qc), _ro(sc)
