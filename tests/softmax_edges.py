"""Rounding-edge inputs for the attention softmax's 1/127 probability grid (helper, no GPU).

Every attention kernel ends its softmax with e = qexp(score - max), p = e / den and
code = rint(p * 127), each with its own shortcut for the quotient.  Random scores put p * 127
within an ulp of a tie k + 1/2 for a few elements in 10^5; the rows built here sit on those
ties.  A row has two live keys: key A holds the row maximum (e_A == 1 exactly), key B lies d
below it, so den = RN(1 + e_B), P_B = e_B / den runs through the codes 0 .. 64 and P_A = 1 / den
through 64 .. 127.  Every other key is dead (masked, or more than 80 below the maximum where the
entry point has no mask): qexp gives exactly 0 there and the denominator keeps its two terms.
The q codes are +-127 on all 64 dims of a head, key A the same signs and key B the opposite
ones, so the accumulators are +-64 * 127^2 and d is steered by one per-token scale alone: the
query's sq at the op-level entry points, key B's cached scale at qtx_decode_attention (whose q
is quantized in the kernel, from a y row with an exactly representable scale).

pool(kind) bisects, for every tie, on the bit pattern of that scale for the float at which the
ORACLE's code flips, and keeps the four floats on each side plus, from a window of +-WINDOW
floats, up to KEEP_PER floats at which each wrong model (MODELS) gets the tie's code wrong.
P depends on the row through the float x = fl(score_B - score_A) alone, so such a sweep visits
every x near the flip: a second free scale reaches no other x.  Two consequences are recorded
here and asserted by tests/test_softmax_edges_ref.py:
  * at the ties EXP_BLIND no float x exists at which an exponential one ulp off changes a code
    of a two-key row (there one step of x moves p * 127 by several ulps past the tie);
  * div_cr with a reciprocal one ulp off is unobservable on these rows: Markstein's correction
    absorbs it, so it is not listed as a model.
The exact ties need no search: n live keys of equal score give p = 1 / n, and 127 / n is a tie
only for n = 2 (63.5, both codes 64: ties-to-even and half-away agree there) and n = 254 (0.5 in
fp32, code 0; a quotient one ulp high or rounding half away gives 1 on all 254 keys); a fully
masked row of 254 keys is the same case at -1e9.  Guard rows put e_B on either side of 2^-60
(div_cr's range) and of EXP_FLUSH; their codes are 0 and 127 either way.

The observed live key carries random nonzero values and the other one zeros, so one code step
moves the context by |v| * s_v / 127 and nothing cancels it.  The case builders below return
what one GPU case feeds to a kernel together with the oracle's view of it; the CPU test checks
the construction and counts, per case, the query rows whose OUTPUT each wrong model changes.

Generation is deterministic and cached.  Measured on the CPU: both pools 1.2 s, the 18 cases
0.8 s, the oracle's expectations of all of them 3.6 s; tests/test_softmax_edges_ref.py as a
whole 12 s."""
import functools

import numpy as np

from oracle import qtx_oracle as O

f32 = np.float32
ACC = 64 * 127 * 127                  # |q . k| of one head: 64 dims of 127 * 127
SEED = 20250611
# op level: the scale of both live keys (sq is swept); a power of two, so the score takes one
# rounding (ACC * sq) and the sweep visits every float x (0.0081 skipped those of the ties 121, 126)
SK_OP = f32(2.0 ** -7)
SQ_DEC = f32(2.0 ** -10)              # decode: q's scale (y = +-127 * SQ_DEC, exact)
# decode: key A's scale (key B's is swept).  score_A = 16129 * 2^-21, a multiple of x's ulp up to
# |x| < 8, so x = fl(score_B - score_A) is exact and the sweep visits every float x
SKA_DEC = f32(2.0 ** -14)
SK_DEAD = f32(1.0)                    # decode self-attention: dead keys score 126 below key A
SV_NEW = f32(2.0 ** -8)               # decode self-attention: the new value row's scale
WINDOW = 4000
KEEP_PER = 3
MODELS = ("recip", "exp+", "exp-", "den+", "den-", "mul_first", "fused")
COUNTED = MODELS[:6]                  # the models every case must catch on 16 rows
EXACT_MODELS = ("half_away", "quot+")
# ties at which no float x = fl(score_B - score_A) lets exp+ or exp- change a code (see above)
EXP_BLIND = (0, 9, 10, 11, 113, 125)
_UP, _DN = f32(np.inf), f32(-np.inf)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------ the softmax and wrong ones
def exps(scores):
    """e = qexp(score - max) as O.softmax_quant forms it."""
    scores = np.asarray(scores, f32)
    return O.qexp(scores - scores.max(axis=-1)[..., None])


def codes_from(e, model=None, total=O.row_sum_lanesplit):
    """rint(p * 127) from the exponentials e [..., Sk] as the oracle (model None) or as a wrong
    model computes it.  total: the denominator's sum over the last axis."""
    e = np.asarray(e, f32)
    if model in ("exp+", "exp-"):     # every computed exponential (not the 0s and the exact 1s)
        e = np.where((e > 0) & (e < 1), np.nextafter(e, _UP if model == "exp+" else _DN), e)
    den = np.asarray(total(e), f32)
    if model in ("den+", "den-"):
        den = np.nextafter(den, _UP if model == "den+" else _DN)
    den = den[..., None]
    c127 = f32(127.0)
    if model == "recip":
        r = np.rint((e * (f32(1.0) / den).astype(f32)) * c127)
    elif model == "mul_first":
        r = np.rint((e * c127) / den)
    elif model == "fused":            # p in float64, one rounding after the multiplication
        r = np.rint((e.astype(np.float64) / den.astype(np.float64) * 127.0).astype(f32))
    elif model == "half_away":
        r = np.floor(((e / den) * c127).astype(np.float64) + 0.5)
    elif model == "quot+":
        p = (e / den).astype(f32)
        r = np.rint(np.where(e > 0, np.nextafter(p, _UP), p) * c127)
    else:
        assert model is None or model in ("exp+", "exp-", "den+", "den-"), model
        r = np.rint((e / den) * c127)
    return r.astype(np.int8)


def model_softmax(model):
    """A drop-in for O.softmax_quant."""
    return lambda scores: codes_from(exps(scores), model)


class patched:
    """O.softmax_quant replaced by a wrong model for the duration of a with block."""

    def __init__(self, model):
        self.fn = model_softmax(model)

    def __enter__(self):
        self.saved, O.softmax_quant = O.softmax_quant, self.fn

    def __exit__(self, *exc):
        O.softmax_quant = self.saved


# ------------------------------------------------------------------ the two-key row
def pair_x(kind, t, bsign=-1):
    """x = fl(score_B - score_A) of a two-key row whose swept scale is t: kind "op" (t = sq,
    both keys' scale SK_OP) or "dec" (t = key B's scale; bsign +1: key B carries key A's signs,
    the only way to bring it within an ulp of key A there)."""
    t = np.asarray(t, f32)
    a, b = f32(ACC), f32(ACC) * f32(bsign)
    if kind == "op":
        sa, sb = ((a * t) * SK_OP) / f32(8.0), ((b * t) * SK_OP) / f32(8.0)
    else:
        sa, sb = ((a * SQ_DEC) * SKA_DEC) / f32(8.0), ((b * SQ_DEC) * t) / f32(8.0)
    return (sb - sa).astype(f32)


def pair_codes(x, model=None):
    """(code_B, code_A) of two-key rows from x, as int arrays."""
    x = np.asarray(x, f32)
    e = np.stack([O.qexp(x), np.ones_like(x)], -1)
    c = codes_from(e, model, total=lambda v: v[..., 0] + v[..., 1])
    return c[..., 0].astype(int), c[..., 1].astype(int)


def _bits(v):
    return int(np.array(v, f32).view(np.int32))


def _floats(bits):
    return np.asarray(bits, np.int32).view(f32)


def _bisect(pred, lo, hi):
    """The smallest bit pattern in (lo, hi] at which pred holds (pred(lo) false, pred(hi) true)."""
    assert not pred(_floats(lo)) and pred(_floats(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(_floats(mid)):
            hi = mid
        else:
            lo = mid
    return hi


def _tie_spec(kind, tie):
    """(key, bsign, lo, hi, pred) of a tie: key 0 (B) for the ties 0 .. 63, key 1 (A) above; the
    sweep's bit range and the predicate that holds at its upper end."""
    key = 0 if tie <= 63 else 1
    if kind == "dec" and tie == 63:       # B just below A: the same signs, its scale up to A's
        return key, +1, _bits(SKA_DEC / f32(2)), _bits(SKA_DEC), lambda c: c >= 64
    lo, hi = _bits(1e-12), _bits(0.05 if kind == "op" else 1.0)
    if key == 0:
        return key, -1, lo, hi, lambda c: c <= tie
    return key, -1, lo, hi, lambda c: c >= tie + 1


@functools.lru_cache(maxsize=None)
def pool(kind):
    """The kept rows of every tie 0 .. 126 as a dict of read-only arrays [n]: t (the swept
    scale), bsign, tie, key (whose code the tie is on: 0 B, 1 A; that key is the observed one),
    side (0 / 1: that key's code is tie + side), near (the float next to the flip on its
    side), code_b, code_a (the oracle's) and bad [n, len(MODELS)] (the model gets the
    tie's key wrong)."""
    rec = []
    for tie in range(127):
        key, bsign, lo, hi, pred = _tie_spec(kind, tie)
        at = lambda t: pair_codes(pair_x(kind, t, bsign))[key]
        flip = _bisect(lambda t: bool(pred(at(t))), lo, hi)
        top = hi if bsign > 0 else flip + WINDOW          # (bsign +1: B stays below A)
        bits = np.arange(flip - WINDOW, min(flip + WINDOW, top + 1), dtype=np.int64)
        x = pair_x(kind, _floats(bits), bsign)
        ref = pair_codes(x)
        keep = set(range(flip - 4, min(flip + 4, top + 1)))
        bad = np.stack([pair_codes(x, m)[key] != ref[key] for m in MODELS], -1)
        order = np.argsort(np.abs(bits - flip + 0.5), kind="stable")      # nearest first
        for m in range(len(MODELS)):
            keep.update(int(bits[i]) for i in order[bad[order, m]][:KEEP_PER])
        for b in sorted(keep):
            i = b - int(bits[0])
            side = int(ref[key][i]) - tie
            assert side in (0, 1), (kind, tie, side)
            rec.append((b, bsign, tie, key, side, b in (flip - 1, flip), ref[0][i], ref[1][i])
                       + tuple(bad[i]))
    a = np.array(rec, np.int64)
    out = dict(t=_floats(a[:, 0]), bsign=a[:, 1], tie=a[:, 2], key=a[:, 3], side=a[:, 4],
               near=a[:, 5].astype(bool), code_b=a[:, 6], code_a=a[:, 7],
               bad=a[:, 8:].astype(bool))
    return {k: _ro(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def guard_t(kind):
    """The swept scales of the guard rows: two floats on each side of e_B = 2^-60 and of
    EXP_FLUSH (e_B == 0 from there on), ascending."""
    lo, hi = _bits(1e-6), _bits(0.05 if kind == "op" else 1.0)
    e_at = lambda t: O.qexp(pair_x(kind, t))
    out = []
    for pred in (lambda t: bool(e_at(t) < f32(2.0 ** -60)), lambda t: bool(e_at(t) == 0)):
        f = _bisect(pred, lo, hi)
        out += [f - 2, f - 1, f, f + 1]
    return _ro(_floats(np.array(out)))


def select(kind, n, salt=0, quota=20):
    """n pool rows for one case (indices, ascending): of every tie the float next to the flip
    on each side and a row that catches exp+ or exp- (where one exists), `quota` rows of every
    counted model, then others; salt rotates which ones."""
    p = pool(kind)
    N = len(p["t"])
    have = set(np.flatnonzero(p["near"]))
    exp_bad = p["bad"][:, 1] | p["bad"][:, 2]
    for tie in range(127):
        c = np.flatnonzero(exp_bad & (p["tie"] == tie))
        if len(c) and not have & set(c):
            have.add(c[salt % len(c)])
    for m in range(len(COUNTED)):
        c = np.flatnonzero(p["bad"][:, m])
        c = np.roll(c, -((salt * 7) % len(c)))
        got = sum(1 for i in c if i in have)
        for i in c:
            if got >= quota:
                break
            if i not in have:
                have.add(i)
                got += 1
    rest = np.roll(np.arange(N), -((salt * 131) % N))
    for i in rest:
        if len(have) >= n:
            break
        have.add(int(i))
    assert len(have) <= n, (len(have), n)
    return np.array(sorted(have))


# ------------------------------------------------------------------ case layouts
def _signs(rng):
    """One head's +-1 pattern on all eight heads."""
    return np.tile(rng.choice(np.array([-1, 1]), 64), 8)


def _nonzero(rng, shape):
    v = rng.integers(-127, 127, shape, dtype=np.int8)          # -127 .. 126 -> -127 .. -1, 1 .. 127
    return (v + (v >= 0)).astype(np.int8)


def _rows(kind, idx, n_guard=0):
    """(t, bsign, obs, src, guard_t) of the rows a case uses: the pool rows idx (src = pool
    index) with the first n_guard guard rows (src = -1 - their index in guard_t) appended."""
    p = pool(kind)
    t, bs, obs, src = p["t"][idx], p["bsign"][idx], p["key"][idx], np.asarray(idx)
    g = guard_t(kind)
    if n_guard:
        t = np.concatenate([t, g[:n_guard]])
        bs = np.concatenate([bs, -np.ones(n_guard, np.int64)])
        obs = np.concatenate([obs, np.arange(n_guard) % 2])
        src = np.concatenate([src, -1 - np.arange(n_guard)])
    return t, bs, obs, src, g


def _arrange(t, bs, obs, src, Sq, guard=None, by_obs=True):
    """Rows into sentences of Sq queries with one observed key each: each group is filled up
    with its own rows again.  guard: (t, src) of the row put in front of every 15 rows.
    Returns t, bsign, src [B, Sq] and obs [B]."""
    out = []
    for o in ((0, 1) if by_obs else (None,)):
        sel = np.flatnonzero(obs == o) if by_obs else np.arange(len(t))
        if not len(sel):
            continue
        tt, bb, ss = list(t[sel]), list(bs[sel]), list(src[sel])
        if guard is not None:
            n = len(tt)
            for at in range(0, n + n // 15 + 1, 16):
                tt.insert(at, guard[0]); bb.insert(at, -1); ss.insert(at, guard[1])
        n = -(-len(tt) // Sq) * Sq
        pick = np.arange(n) % len(tt)
        out.append((np.array(tt, f32)[pick].reshape(-1, Sq), np.array(bb)[pick].reshape(-1, Sq),
                    np.array(ss)[pick].reshape(-1, Sq), np.full(n // Sq, 0 if o is None else o)))
    return tuple(np.concatenate([g[i] for g in out]) for i in range(4))


def op_case(idx, Sk, Sq, mode, seed, n_guard=8, guard_every=0, by_obs=True):
    """An op-level attention case (qtx_attention_i8 / _trace / _i8_quant) on the "op" pool rows
    idx.  mode "row": a mask row per query ([B, Sq, Sk], m_is = Sk); the A / B patterns
    alternate over the key positions (A on the even ones in even sentences, on the odd ones in
    odd sentences) and each query keeps its own pair.  mode "key": one key mask per sentence
    ([B, Sk], m_is = 0), the pair moves from sentence to sentence and the masked keys are
    random.  by_obs False (the trace, whose codes are compared directly): every value random."""
    rng = np.random.default_rng(SEED + seed)
    t, bs, obs, src, g = _rows("op", idx, n_guard)
    # guard_every = 16: a guard row with 0 < e_B < 2^-60 in front of every 15 rows, so every
    # wave of k_attn_mfma takes the true division
    guard = (g[3], -4) if guard_every else None
    sq, _, src, obs = _arrange(t, bs, obs, src, Sq, guard, by_obs)
    B = len(sq)
    sgn = np.stack([_signs(rng) for _ in range(B)])
    q = np.repeat((sgn * 127)[:, None, :], Sq, 1).astype(np.int8)
    bi, ii = np.arange(B)[:, None], np.arange(Sq)[None, :]
    if mode == "row":
        par = (np.arange(B) & 1)[:, None]                         # parity of the A positions
        nA, nB = (Sk + 1 - par) // 2, (Sk + par) // 2
        jA = 2 * ((ii + 3 * bi) % nA) + par
        jB = 2 * ((37 * ii + 5 * bi + 5) % nB) + (1 - par)
        isA = (np.arange(Sk)[None, :] & 1) == par
        k = np.where(isA[..., None], sgn[:, None, :], -sgn[:, None, :]) * 127
        mask = np.zeros((B, Sq, Sk), np.uint8)
        mask[bi, ii, jA] = 1
        mask[bi, ii, jB] = 1
        live_obs = isA == (obs[:, None] == 1)
        m_bs, m_is, mdev = Sq * Sk, Sk, mask
    else:
        b = np.arange(B)          # key 16 kt + 4 e + fg: every kt, e and fg within 8 sentences
        jA1 = (16 * (b % 8) + 4 * ((b + b // 8) % 4) + (b + 1) % 4) % Sk
        jB1 = (16 * ((b + 3) % 8) + 4 * ((b + 2 + b // 8) % 4) + (b + 3) % 4) % Sk
        if Sk < 128:              # a small sentence: step through its keys
            jA1 = (7 * b + 1) % Sk
            jB1 = (jA1 + 1 + (b // Sk) % (Sk - 1)) % Sk
        assert np.all(jA1 != jB1)
        k = rng.integers(-127, 128, (B, Sk, 512))
        k[np.arange(B), jA1], k[np.arange(B), jB1] = sgn * 127, -sgn * 127
        km = np.zeros((B, Sk), np.uint8)
        km[np.arange(B), jA1] = km[np.arange(B), jB1] = 1
        jA, jB = np.repeat(jA1[:, None], Sq, 1), np.repeat(jB1[:, None], Sq, 1)
        mask = np.repeat(km[:, None, :], Sq, 1)
        live_obs = np.zeros((B, Sk), bool)
        live_obs[np.arange(B), np.where(obs == 1, jA1, jB1)] = True
        live_obs |= km == 0                                       # masked keys: random values
        m_bs, m_is, mdev = Sk, 0, km
    v = _nonzero(rng, (B, Sk, 512))
    if by_obs:
        v = np.where(live_obs[..., None], v, 0).astype(np.int8)
    view = dict(q=q, sq=sq.astype(f32), k=k.astype(np.int8), sk=np.full((B, Sk), SK_OP, f32), v=v,
                sv=rng.uniform(0.002, 0.03, (B, Sk)).astype(f32), mask=mask)
    return dict(view={n: _ro(a) for n, a in view.items()}, jA=_ro(jA), jB=_ro(jB),
                obs=_ro(np.repeat(obs[:, None], Sq, 1)), src=_ro(src), kind="op",
                mask_dev=_ro(mdev), m_bs=m_bs, m_is=m_is, pairs=True, by_obs=by_obs)


def exact_case(Sk=254, reps=2):
    """The exact ties, mode "row", every key with key A's pattern and scale: query 3 r keeps two
    keys (n = 2), query 3 r + 1 all Sk (n = 254), query 3 r + 2 none (fully masked)."""
    rng = np.random.default_rng(SEED + 254)
    Sq = 3 * reps
    sgn = _signs(rng)[None]
    q = np.repeat((sgn * 127)[:, None, :], Sq, 1).astype(np.int8)
    k = np.repeat((sgn * 127)[:, None, :], Sk, 1).astype(np.int8)
    mask = np.zeros((1, Sq, Sk), np.uint8)
    n = np.zeros((1, Sq), np.int64)
    for r in range(reps):
        mask[0, 3 * r, [(29 * r + 3) % Sk, (71 * r + 130) % Sk]] = 1
        mask[0, 3 * r + 1] = 1
        n[0, 3 * r: 3 * r + 3] = (2, Sk, Sk)
    view = dict(q=q, sq=rng.uniform(0.002, 0.03, (1, Sq)).astype(f32), k=k,
                sk=np.full((1, Sk), SK_OP, f32), v=_nonzero(rng, (1, Sk, 512)),
                sv=rng.uniform(0.002, 0.03, (1, Sk)).astype(f32), mask=mask)
    return dict(view={a: _ro(b) for a, b in view.items()}, n=_ro(n), kind="op", mask_dev=_ro(mask),
                m_bs=Sq * Sk, m_is=Sk, pairs=False, by_obs=True)


def _dec_slots(S):
    """Key positions a decode case moves its pair over: a lane's first and second slot, the
    fragment borders, the last keys before S and the first key of the last 16-group."""
    c = {0, 1, 5, 15, 16, 31, 47, 48, 63, 64, 65, 69, 100, 127, S - 1, S - 2, 16 * ((S - 1) // 16)}
    return np.array(sorted(j for j in c if 0 <= j < S))


def _dec_pair(B, S):
    c = _dec_slots(S)
    b = np.arange(B)
    if len(c) == 1:
        return c[b * 0], c[b * 0]
    return c[b % len(c)], c[(b + 1 + (b // len(c)) % (len(c) - 1)) % len(c)]


def cross_case(idx, S, seed):
    """qtx_decode_attention with kv_new = 0 on the "dec" pool rows idx: one query per sentence,
    y = +-127 * SQ_DEC, key A with SKA_DEC, key B with the swept scale, everything else masked
    (random codes, scales and values there)."""
    rng = np.random.default_rng(SEED + seed)
    t, bs, obs, src, _ = _rows("dec", idx, 8)
    B = len(t)
    sgn = np.stack([_signs(rng) for _ in range(B)])
    y = (sgn * (f32(127.0) * SQ_DEC)).astype(f32)
    jA, jB = _dec_pair(B, S)
    b = np.arange(B)
    kc = rng.integers(-127, 128, (B, S, 512), dtype=np.int8)
    kc[b, jA], kc[b, jB] = sgn * 127, sgn * (127 * bs)[:, None]
    skc = rng.uniform(0.002, 0.03, (B, S)).astype(f32)
    skc[b, jA], skc[b, jB] = SKA_DEC, t
    vc = _nonzero(rng, (B, S, 512))
    vc[b, np.where(obs == 1, jB, jA)] = 0                        # the live key not observed
    mask = np.zeros((B, S), np.uint8)
    mask[b, jA] = mask[b, jB] = 1
    raw = dict(y=y, kc=kc.astype(np.int8), vc=vc, skc=skc,
               svc=rng.uniform(0.002, 0.03, (B, S)).astype(f32), mask=mask)
    qq, sq = O.quant_rows(y)
    view = dict(q=qq[:, None], sq=sq[:, None], k=raw["kc"], sk=skc, v=vc, sv=raw["svc"],
                mask=mask[:, None])
    return dict(view={n: _ro(a) for n, a in view.items()}, raw={n: _ro(a) for n, a in raw.items()},
                jA=_ro(jA[:, None]), jB=_ro(jB[:, None]), obs=_ro(obs[:, None]),
                src=_ro(src[:, None]), kind="dec", pairs=True, by_obs=True, dec=True)


def self_case(idx, step, seed, kv_bs=128):
    """qtx_decode_attention with kv_new = 1 at position `step` on the "dec" pool rows idx: no
    mask, so the dead keys carry key B's signs and SK_DEAD (126 below key A).  In the even
    sentences (in all of them at step 1) the new key is key A: y's k third is +-127 * SKA_DEC;
    in the odd ones it is a dead key.  The new value row is integers times SV_NEW with one 127
    (zeros where the new key is the live key not observed).  Cache rows past `step` are random."""
    rng = np.random.default_rng(SEED + seed)
    t, bs, obs, src, _ = _rows("dec", idx, 8)
    B, n = len(t), step + 1
    b = np.arange(B)
    sgn = np.stack([_signs(rng) for _ in range(B)])
    new_a = (b % 2 == 0) | (step < 2)
    pa, pb = _dec_pair(B, step)                                  # among the cached keys
    jA = np.where(new_a, step, pa)
    jB = np.where(new_a, pb if step > 1 else 0, pb)
    jB = np.where(jB == jA, pa, jB)
    assert np.all(jA != jB) and np.all(jB < step)
    kc = rng.integers(-127, 128, (B, kv_bs, 512), dtype=np.int8)
    skc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
    kc[:, :n], skc[:, :n] = (-sgn * 127)[:, None, :], SK_DEAD
    kc[b, jA], skc[b, jA] = sgn * 127, SKA_DEC
    kc[b, jB], skc[b, jB] = sgn * (127 * bs)[:, None], t
    vc = _nonzero(rng, (B, kv_bs, 512))
    vc[b, np.where(obs == 1, jB, jA)] = 0
    svc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
    svc[:, step] = SV_NEW
    vc[b, step, rng.integers(0, 512, B)] = np.where(vc[b, step, 0] == 0, 0, 127)
    y = np.empty((B, 1536), f32)
    y[:, :512] = sgn * (f32(127.0) * SQ_DEC)
    y[:, 512:1024] = kc[:, step].astype(f32) * skc[:, step, None]   # exact: +-127 * 2^e
    y[:, 1024:] = vc[:, step].astype(f32) * SV_NEW
    stale = rng.integers(-127, 128, (B, 512)).astype(np.int8)
    raw = dict(y=y, kc=kc.astype(np.int8), vc=vc.copy(), skc=skc.copy(), svc=svc.copy())
    raw["kc"][:, step], raw["vc"][:, step] = stale, stale[:, ::-1]     # what the step overwrites
    raw["skc"][:, step] = raw["svc"][:, step] = f32(0.5)
    qq, sq = O.quant_rows(y[:, :512])
    qk, sk = O.quant_rows(y[:, 512:1024])
    qv, sv = O.quant_rows(y[:, 1024:])
    after = dict(kc=raw["kc"].copy(), vc=raw["vc"].copy(), skc=raw["skc"].copy(), svc=raw["svc"].copy())
    after["kc"][:, step], after["vc"][:, step] = qk, qv
    after["skc"][:, step], after["svc"][:, step] = sk, sv
    view = dict(q=qq[:, None], sq=sq[:, None], k=after["kc"][:, :n], sk=after["skc"][:, :n],
                v=after["vc"][:, :n], sv=after["svc"][:, :n], mask=np.ones((B, 1, n), np.uint8))
    return dict(view={a: _ro(c) for a, c in view.items()}, raw={a: _ro(c) for a, c in raw.items()},
                after={a: _ro(c) for a, c in after.items()}, step=step, kv_bs=kv_bs,
                intended=dict(kc=_ro(kc[:, step].astype(np.int8)), skc=_ro(skc[:, step]),
                              vc=_ro(vc[:, step]), new_a=_ro(new_a)),
                jA=_ro(jA[:, None]), jB=_ro(jB[:, None]), obs=_ro(obs[:, None]),
                src=_ro(src[:, None]), kind="dec", pairs=True, by_obs=True, dec=True)


# ------------------------------------------------------------------ the cases
# name -> (entry point, builder).  The trace takes every kept row; the other cases take
# select()ions of the pool (each with every tie on both sides and its model quotas), sized so
# that the oracle's PV chain over all their keys stays a fraction of a second.
def _all(kind):
    return np.arange(len(pool(kind)["t"]))


CASES = {
    "trace16": ("trace", lambda: op_case(_all("op"), 16, len(_all("op")) + 8, "row", 1, by_obs=False)),
    "trace254": ("trace", lambda: exact_case()),
    "i8_128": ("i8", lambda: op_case(select("op", 280, 1), 128, 72, "row", 2)),
    "i8_20": ("i8", lambda: op_case(select("op", 472, 2), 20, 40, "key", 3)),
    "i8_130": ("i8", lambda: op_case(select("op", 280, 3), 130, 72, "row", 4)),
    "i8_254": ("i8", lambda: op_case(select("op", 280, 4), 254, 72, "row", 5)),
    "i8_254x": ("i8", lambda: exact_case()),
    "i8_guard": ("i8", lambda: op_case(select("op", 280, 5), 128, 80, "row", 6, guard_every=16)),
    "encq128": ("i8_quant", lambda: op_case(select("op", 1016, 6), 128, 128, "key", 7)),
    "encq16": ("i8_quant", lambda: op_case(select("op", 504, 7), 16, 16, "key", 8)),
    "cross17": ("cross", lambda: cross_case(select("dec", 504, 1), 17, 9)),
    "cross64": ("cross", lambda: cross_case(select("dec", 280, 2), 64, 10)),
    "cross65": ("cross", lambda: cross_case(select("dec", 280, 3), 65, 11)),
    "cross128": ("cross", lambda: cross_case(select("dec", 280, 4), 128, 12)),
    "self1": ("self", lambda: self_case(select("dec", 504, 5), 1, 13, kv_bs=8)),
    "self63": ("self", lambda: self_case(select("dec", 280, 6), 63, 14)),
    "self64": ("self", lambda: self_case(select("dec", 280, 7), 64, 15)),
    "self127": ("self", lambda: self_case(select("dec", 280, 8), 127, 16)),
}


def names(entry):
    return [n for n, (e, _) in CASES.items() if e == entry]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][1]()


@functools.lru_cache(maxsize=None)
def expected(name, dec=False):
    """The oracle's (context [B, Sq, 512], codes [B, 8, Sq, Sk]) of a case."""
    c = case(name)
    v = c["view"]
    ctx, qp = O.attention(v["q"], v["sq"], v["k"], v["sk"], v["v"], v["sv"], v["mask"], 8,
                          dec=bool(c.get("dec", dec)))
    return _ro(ctx), _ro(qp)


def expected_quant(name):
    """The oracle's (codes, scales) of the per-token-quantized context."""
    qc, sc = O.quant_rows(expected(name, False)[0])
    return _ro(qc), _ro(sc)


@functools.lru_cache(maxsize=None)
def case_exps(name):
    """e [B, 8, Sq, Sk] of a case (what every model starts from)."""
    v = case(name)["view"]
    return _ro(exps(O.attention_scores(O.split_heads(v["q"], 8), v["sq"], O.split_heads(v["k"], 8),
                                       v["sk"], v["mask"])))


@functools.lru_cache(maxsize=None)
def changed_all(name, dec, output, models):
    """{model: bool [B, Sq]}: the query rows whose output changes when O.softmax_quant is the
    model.  output "ctx": the fp32 context; "quant": ctx8 and sctx; "codes": p_codes.  Only the
    rows whose codes change go through the PV chain again (equal codes give equal outputs),
    those of all models in common batches."""
    c = case(name)
    v = c["view"]
    ctx, qp = expected(name, dec)
    alt = np.stack([codes_from(case_exps(name), m) for m in models])
    diff = (alt != qp[None]).any(axis=(2, 4))                   # [M, B, Sq]
    if output == "codes":
        return dict(zip(models, diff))
    out = np.zeros_like(diff)
    first = {}                                # models that give a row the same codes share its run
    for m, b, i in np.argwhere(diff):
        first.setdefault((b, i, alt[m, b, :, i].tobytes()), []).append(m)
    where = np.array([(ms[0], b, i) for (b, i, _), ms in first.items()]).reshape(-1, 3)
    res = np.zeros(len(where), bool)
    v4 = O.split_heads(v["v"], 8)
    for lo in range(0, len(where), 160):
        m, b, i = where[lo:lo + 160].T
        got = O.merge_heads(O.attention_pv(alt[m, b, :, i][:, :, None, :], v4[b], v["sv"][b], dec))[:, 0]
        if output == "quant":
            (qa, sa), (qb, sb) = O.quant_rows(got), O.quant_rows(ctx[b, i])
            res[lo:lo + 160] = (qa != qb).any(-1) | (sa != sb)
        else:
            res[lo:lo + 160] = (got != ctx[b, i]).any(-1)
    for r, ((b, i, _), ms) in zip(res, first.items()):
        out[ms, b, i] = r
    return dict(zip(models, out))


def changed_rows(name, model, dec=False, output="ctx"):
    """bool [B, Sq] of one model (changed_all over MODELS, or over EXACT_MODELS)."""
    dec = bool(case(name).get("dec", dec))
    group = MODELS if model in MODELS else EXACT_MODELS
    return changed_all(name, dec, output, group)[model]


OUTPUT = {"trace": "codes", "i8": "ctx", "i8_quant": "quant", "cross": "ctx", "self": "ctx"}
