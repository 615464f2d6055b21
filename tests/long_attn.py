"""Directed inputs for k_dec_attn_long's per-key paths (a helper module, no GPU): every key slot
of the cross-attention and every step of the self-attention, each with a closed-form
expectation.  Shared by tests/test_gpu_long_fused.py (GPU == these, bit for bit) and
tests/test_long_attn_ref.py (the closed forms == O.attention).

Random caches give most of 512 keys P == 0, so a wrong value byte, group dword, clamp or scale
of one key slot shows by chance alone.  Here one key holds P == 127 / 127 and every other key
exactly 0, so the context is that key's value row times its scale: RN(RN(1 * s_v) * v).

one_hot(S)     B = S sentences of S keys, sentence b keeps key b alone (cross-attention).
EveryStep      B = 2 sentences at kv_bs = 512 over the steps 0 .. 511 of one pair of caches.
               q is +-127 * 2^-10 on every dim; a dead key carries the opposite signs and scale 1
               (126 below a live one, as softmax_edges.self_case builds them), a live key q's
               signs and scale 2^-14.  Sentence 0: the new key is the only live one.  Sentence 1
               (from step 1 on): the live key is the cached key j(step) = (37 step + 5) % 509 % step
               and the new key is dead, so the context is a value row appended `step - j` steps
               earlier.  before(step) names the rows the test rewrites ahead of the call: the
               live key of sentence 1, the rows that were live at the step before, and stale
               codes and scales at row `step`, which the append must replace and the attention
               must not see.
"""
import numpy as np

from oracle import qtx_oracle as O

f32 = np.float32
SQ, SK_LIVE, SK_DEAD = f32(2.0 ** -10), f32(2.0 ** -14), f32(1.0)
SK_STALE, SV_STALE = f32(64.0), f32(7.0)      # a stale key would outscore every live one
KV_BS = 512


def attention_chunked(qq, sq, kc, skc, vc, svc, mask, chunk=32):
    """O.attention(dec=True) of one-query sentences, `chunk` sentences at a time (its int64
    operands of 512 sentences of 512 keys would take a gigabyte)."""
    out = [O.attention(qq[s, None], sq[s, None], kc[s], skc[s], vc[s], svc[s], mask[s, None], dec=True)
           for s in (slice(lo, lo + chunk) for lo in range(0, len(qq), chunk))]
    return np.concatenate([o[0][:, 0] for o in out]), np.concatenate([o[1][:, :, 0] for o in out])


def nonzero(rng, shape):
    v = rng.integers(-127, 127, shape, dtype=np.int8)            # -127 .. -1, 1 .. 127
    v += v >= 0
    return v


def one_hot(S):
    """dict(y, kc, vc, skc, svc, mask, ctx): ctx[b] = RN(s_v[b, b] * v[b, b]), asserted here
    against nothing: tests/test_long_attn_ref.py and the GPU test compare it with O.attention."""
    rng = np.random.default_rng(8000 + S)
    y = rng.standard_normal((S, 512)).astype(f32)
    kc = rng.integers(-127, 128, (S, S, 512), dtype=np.int8)
    vc = nonzero(rng, (S, S, 512))
    skc = rng.uniform(0.002, 0.03, (S, S)).astype(f32)
    svc = rng.uniform(0.002, 0.03, (S, S)).astype(f32)
    b = np.arange(S)
    ctx = ((f32(1.0) * svc[b, b])[:, None] * vc[b, b].astype(f32)).astype(f32)
    return dict(y=y, kc=kc, vc=vc, skc=skc, svc=svc, mask=np.eye(S, dtype=np.uint8), ctx=ctx)


class EveryStep:
    """The 512 steps' inputs and closed-form results, [step, sentence, ...]: y [512, 2, 1536],
    the appended rows qk / qv [512, 2, 512] and sk / sv [512, 2], ctx [512, 2, 512], the stale
    rows stale_k / stale_v, and j [512] (sentence 1's live cached key; -1 at step 0, where its
    new key is live as sentence 0's is)."""

    def __init__(self, seed=9000):
        rng = np.random.default_rng(seed)
        n = KV_BS
        self.sgn = np.stack([np.tile(rng.choice(np.array([-1, 1]), 64), 8) for _ in range(2)])
        # ((37 s + 5) % s alone is 5 for every s > 5: the residues of the prime 509 first)
        self.j = np.array([-1] + [(37 * s + 5) % 509 % s for s in range(1, n)])
        y = np.empty((n, 2, 1536), f32)
        y[:, :, :512] = self.sgn * (f32(127.0) * SQ)
        y[:, 0, 512:1024] = self.sgn[0] * (f32(127.0) * SK_LIVE)
        y[1:, 1, 512:1024] = -self.sgn[1] * (f32(127.0) * SK_DEAD)
        y[0, 1, 512:1024] = self.sgn[1] * (f32(127.0) * SK_LIVE)
        y[:, :, 1024:] = rng.standard_normal((n, 2, 512)) * rng.uniform(0.1, 4.0, (n, 2, 1))
        self.y = y
        self.qk, self.sk = O.quant_rows(y[:, :, 512:1024])
        self.qv, self.sv = O.quant_rows(y[:, :, 1024:])
        assert np.all(np.abs(self.qk) == 127) and set(np.unique(self.sk)) == {SK_LIVE, SK_DEAD}
        self.dead = (-self.sgn * 127).astype(np.int8)            # [2, 512]
        self.live = (self.sgn * 127).astype(np.int8)
        self.stale_k = np.repeat(self.live[None], n, 0)          # q's signs, SK_STALE
        self.stale_v = nonzero(rng, (n, 2, 512))
        ctx = (self.sv[..., None] * self.qv.astype(f32)).astype(f32)        # the new value row
        jj = self.j[1:]
        ctx[1:, 1] = (self.sv[jj, 1, None] * self.qv[jj, 1].astype(f32)).astype(f32)
        self.ctx = ctx

    def before(self, step):
        """[(sentence, row, k codes, k scale)] to write ahead of the call, in order; row `step`
        also takes stale_v[step] and SV_STALE."""
        w = []
        if step > 0:
            w.append((0, step - 1, self.dead[0], SK_DEAD))       # sentence 0's last new key
            if self.j[step - 1] >= 0:
                w.append((1, self.j[step - 1], self.dead[1], SK_DEAD))
            else:
                w.append((1, 0, self.dead[1], SK_DEAD))          # (its new key of step 0)
            w.append((1, self.j[step], self.live[1], SK_LIVE))
        return w + [(b, step, self.stale_k[step, b], SK_STALE) for b in range(2)]

    def view(self, step):
        """The oracle's operands (qq, sq, k, sk, v, sv, mask) of the step, after the append."""
        n = step + 1
        k = np.repeat(self.dead[:, None], n, 1)
        skc = np.full((2, n), SK_DEAD, f32)
        k[0, step], skc[0, step] = self.live[0], SK_LIVE
        jl = self.j[step] if step else 0
        k[1, jl], skc[1, jl] = self.live[1], SK_LIVE
        np.testing.assert_array_equal(k[:, step], self.qk[step])
        np.testing.assert_array_equal(skc[:, step], self.sk[step])
        qq, sq = O.quant_rows(self.y[step, :, :512])
        v = np.ascontiguousarray(self.qv[:n].transpose(1, 0, 2))
        return qq, sq, k, skc, v, np.ascontiguousarray(self.sv[:n].T), np.ones((2, n), np.uint8)
