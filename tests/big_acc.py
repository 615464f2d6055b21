"""Operands whose integer GEMM accumulators reach 2^24 and beyond (a helper module).

The contract is y = ((float(acc) * s_a) * s_w) + b.  For |acc| >= 2^24 the
conversion float(acc) rounds: in [2^24, 2^25) the fp32 spacing is 2, so every odd
accumulator is an exact tie, on which round-to-nearest-even (the oracle's astype(float32)),
truncation and round-half-away give different floats.  K * 127^2 crosses 2^24 at K >= 1041,
but random codes never come near it (the sum of K products of independent signs grows like
sqrt(K)); the codes here share one sign pattern along K, so the products of an activation
row and a weight row are nearly all positive and |acc| is about K * mean|a| * mean|w|.
"""
import numpy as np

f32 = np.float32
TWO24 = 1 << 24
X_SCALE = f32(2.0 ** -4)


def shared_signs(K):
    """The +1 / -1 pattern along K that every correlated_codes() of this K starts from
    (fixed by K alone: activations and weights must agree on it)."""
    return np.where(np.random.default_rng([0x5167, K]).integers(0, 2, K) == 1, 1, -1).astype(np.int32)


def correlated_codes(rng, R, K, lo, flip):
    """[R, K] int8 codes: magnitude uniform in [lo, 127], sign = shared_signs(K) with each
    element's sign flipped with probability `flip`; every row holds at least one |code| = 127
    (so a per-row absmax quantizer of code * 2^-4 finds the scale 2^-4 exactly)."""
    mag = rng.integers(lo, 128, (R, K)).astype(np.int32)
    mag[np.arange(R), rng.integers(0, K, R)] = 127
    sign = shared_signs(K)[None, :] * np.where(rng.uniform(size=(R, K)) < flip, -1, 1)
    return (mag * sign).astype(np.int8)


def negate_half(qw):
    """The weight codes with every odd row negated: half of the outputs large and negative."""
    out = np.array(qw, np.int8)
    out[1::2] = -out[1::2]
    return out


def as_fp32(codes):
    """x = code * 2^-4, exact in fp32.  The per-token quantizer (oracle quant_rows) returns
    exactly `codes` and the scale 2^-4 for it: max|x| = 127/16 and (127/16) / 127 = 2^-4."""
    return (codes.astype(f32) * X_SCALE).astype(f32)


def operands(seed, M, N, K, lo, flip):
    """The crafted (qx [M, K], qw [N, K] with odd rows negated) of one case."""
    rng = np.random.default_rng(seed)
    return correlated_codes(rng, M, K, lo, flip), negate_half(correlated_codes(rng, N, K, lo, flip))


# (lo, flip) per K: the conditions they meet are stated and checked in test_big_acc_ref.py
PARAMS = {2048: (96, 0.02), 1280: (120, 0.01), 1344: (120, 0.01)}
SEED = 1


def to_float_trunc(acc):
    """float(acc) rounded toward zero (what a truncating conversion would give)."""
    a = np.asarray(acc, np.int64)
    r = a.astype(f32)
    over = np.abs(r.astype(np.float64)) > np.abs(a)
    return np.where(over, np.nextafter(r, f32(0)), r).astype(f32)


def to_float_half_away(acc):
    """float(acc) rounded to nearest, ties away from zero."""
    a = np.asarray(acc, np.int64)
    t = to_float_trunc(a)
    up = np.nextafter(t, np.where(a < 0, f32(-np.inf), f32(np.inf))).astype(f32)
    rem = np.abs(a) - np.abs(t.astype(np.float64)).astype(np.int64)
    gap = (np.abs(up.astype(np.float64)) - np.abs(t.astype(np.float64))).astype(np.int64)
    return np.where(2 * rem >= gap, np.where(rem == 0, t, up), t).astype(f32)


def stats(acc):
    """Shares the reference test asserts (and the docstrings record)."""
    a = np.asarray(acc, np.int64)
    odd = (a & 1) == 1
    big = np.abs(a) >= TWO24
    rne = a.astype(np.int32).astype(f32)
    n_odd = max(int((odd & big).sum()), 1)
    return dict(min_abs=int(np.abs(a).min()), max_abs=int(np.abs(a).max()),
                odd_big=float((odd & big).mean()), negative=float((a < 0).mean()),
                vs_trunc=float(((rne != to_float_trunc(a)) & odd & big).sum() / n_odd),
                vs_half_away=float(((rne != to_float_half_away(a)) & odd & big).sum() / n_odd))
