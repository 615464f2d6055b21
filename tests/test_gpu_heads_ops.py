"""The attention operations for 4 and 16 heads (include/qtx_heads.h: head widths 128 and 32)
against oracle/qtx_oracle.py attention(), bit for bit: k_attn_mfma_hd through
qtx_attention_heads_i8 and k_dec_attn_hd through qtx_decode_attention_heads
(csrc/qtx_attn_heads.hip).  Outputs live in guarded() buffers under both poisons.

Key counts sit on the kernels' edges: 1, a ragged 4-key PV step (5), a full and a just-started
16-key tile (64 / 65), the 128-slot instances' switch (128 / 129) and the most (512)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import POISONS, guarded  # noqa: E402
from test_gpu_model_configs import T_  # noqa: E402
from test_gpu_scored import P  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
HEADS = (4, 16)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def codes(rng, *shape):
    return rng.integers(-127, 128, shape).astype(np.int8)


def scales(rng, *shape):
    return rng.uniform(0.01, 0.035, shape).astype(f32)


def run_attention(torch, H, q, sq, k, sk, v, sv, mask, m_bs, m_is, dec, poison):
    from qtx import _lib
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    ctx, chk = guarded(torch, (B, Sq, 512), torch.float32, poison, name="ctx")
    t = [T_(torch, a) for a in (q, sq, k, sk, v, sv)]
    md = T_(torch, mask.astype(np.uint8)) if mask is not None else None
    _lib.call("qtx_attention_heads_i8", *[P(x) for x in t], P(md), m_bs, m_is, B, H, Sq, Sk,
              P(ctx), dec, 512 // H, C.c_void_p(0))
    torch.cuda.synchronize()
    chk()
    return ctx.cpu().numpy()


def vgroups(v, kv_bs):
    """[B, rows, 512] codes -> the step's 4-key groups [B, ceil(kv_bs / 4), 512, 4]."""
    B, G4 = v.shape[0], (kv_bs + 3) // 4
    pad = np.zeros((B, 4 * G4, 512), np.int8)
    pad[:, :v.shape[1]] = v
    return np.ascontiguousarray(pad.reshape(B, G4, 4, 512).transpose(0, 1, 3, 2))


def pmax_of(ctx):
    return np.abs(ctx.reshape(ctx.shape[0], 8, 64)).max(axis=2).T.copy()   # [8][B]


# ---- qtx_attention_heads_i8 -----------------------------------------------------------------
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("Sq,Sk,dec,causal", [(1, 1, 0, 0), (17, 5, 1, 0), (70, 64, 0, 0), (17, 65, 1, 1),
                                              (70, 129, 1, 0), (70, 129, 0, 1), (17, 512, 0, 0),
                                              (1, 512, 1, 1), (17, 64, 1, 1)])
@pytest.mark.parametrize("H", HEADS)
def test_attention_heads(torch, H, Sq, Sk, dec, causal, poison):
    """Key mask [B, Sk] with sentence 1 fully masked, or the last Sq rows of the causal
    [Sk, Sk] mask shared by the sentences (a row per query, m_is = Sk)."""
    rng = np.random.default_rng(1000 * H + 10 * Sk + Sq)
    B = 3
    q, k, v = codes(rng, B, Sq, 512), codes(rng, B, Sk, 512), codes(rng, B, Sk, 512)
    sq, sk, sv = scales(rng, B, Sq), scales(rng, B, Sk), scales(rng, B, Sk)
    if causal:
        mask = np.ascontiguousarray(np.tril(np.ones((Sk, Sk), np.uint8))[Sk - Sq:])
        om, m_bs, m_is = mask[None], 0, Sk
    else:
        mask = (rng.random((B, Sk)) < 0.8).astype(np.uint8)
        mask[1] = 0
        mask[0, 0] = 1
        om, m_bs, m_is = mask[:, None, :], Sk, 0
    ref, _ = O.attention(q, sq, k, sk, v, sv, om, H, dec=bool(dec))
    got = run_attention(torch, H, q, sq, k, sk, v, sv, mask, m_bs, m_is, dec, poison)
    np.testing.assert_array_equal(got, ref)


# ---- qtx_decode_attention_heads -------------------------------------------------------------
def run_decode(torch, H, kv_new, y, kc, vc, skc, svc, kv_bs, step, S, mask, poison):
    """Returns (ctx, pmax, kc, vc, skc, svc) after the call; the caches are the inputs' copies."""
    from qtx import _lib
    B = y.shape[0]
    ctx, c1 = guarded(torch, (B, 512), torch.float32, poison, name="ctx")
    pm, c2 = guarded(torch, (8, B), torch.float32, poison, name="pmax")
    d = [T_(torch, a) for a in (y, kc, vc, skc, svc)]
    sd = T_(torch, np.array([step, 0, 0, 0], np.int32))
    md = T_(torch, mask.astype(np.uint8)) if mask is not None else None
    _lib.call("qtx_decode_attention_heads", kv_new, P(d[0]), y.shape[1], P(d[1]), P(d[2]), P(d[3]),
              P(d[4]), kv_bs, P(sd), S, P(md), B, P(ctx), P(pm), H, C.c_void_p(0))
    torch.cuda.synchronize()
    c1()
    c2()
    return [x.cpu().numpy() for x in (ctx, pm, d[1], d[2], d[3], d[4])]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("S", [1, 17, 128, 129, 512])
@pytest.mark.parametrize("H", HEADS)
def test_decode_heads_cross(torch, H, S, poison):
    rng = np.random.default_rng(7000 * H + S)
    B = 3
    y = (rng.standard_normal((B, 512)) * 2).astype(f32)
    k, v = codes(rng, B, S, 512), codes(rng, B, S, 512)
    sk, sv = scales(rng, B, S), scales(rng, B, S)
    mask = np.ones((B, S), np.uint8)
    for b in range(B):                       # ragged: sentence b keeps its first keys
        mask[b, max(1, S - 5 * b):] = 0 if b else 1
    q, sq = O.quant_rows(y, 8)
    ref, _ = O.attention(q[:, None], sq[:, None], k, sk, v, sv, mask[:, None, :], H, dec=True)
    ctx, pm, kc2, vc2, sk2, sv2 = run_decode(torch, H, 0, y, k, vgroups(v, S), sk, sv, S, 0, S, mask, poison)
    np.testing.assert_array_equal(ctx, ref[:, 0])
    np.testing.assert_array_equal(pm, pmax_of(ref[:, 0]))
    np.testing.assert_array_equal(kc2, k)
    np.testing.assert_array_equal(vc2, vgroups(v, S))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("step", [0, 3, 4, 127, 128, 511])
@pytest.mark.parametrize("H", HEADS)
def test_decode_heads_self(torch, H, step, poison):
    """The append at `step` in a cache of kv_bs = step + 9 rows (512 at step 511: the entry's
    most), stale codes and scales planted at row `step`; context, pmax and both caches whole."""
    rng = np.random.default_rng(9000 * H + step)
    B, kv_bs = 3, min(step + 9, 512)
    y = (rng.standard_normal((B, 1536)) * 2).astype(f32)
    k, v = codes(rng, B, kv_bs, 512), codes(rng, B, kv_bs, 512)    # row `step` on: stale
    sk, sv = scales(rng, B, kv_bs), scales(rng, B, kv_bs)
    sk[:, step], sv[:, step] = 1e6, -1e6
    (q, sq), (kn, skn), (vn, svn) = (O.quant_rows(y[:, 512 * i:512 * i + 512], 8) for i in range(3))
    ek, ev, esk, esv = k.copy(), v.copy(), sk.copy(), sv.copy()
    ek[:, step], ev[:, step], esk[:, step], esv[:, step] = kn, vn, skn, svn
    n = step + 1
    ref, _ = O.attention(q[:, None], sq[:, None], ek[:, :n], esk[:, :n], ev[:, :n], esv[:, :n],
                         np.ones((B, 1, n)), H, dec=True)
    ctx, pm, kc2, vc2, sk2, sv2 = run_decode(torch, H, 1, y, k, vgroups(v, kv_bs), sk, sv, kv_bs, step,
                                             0, None, poison)
    np.testing.assert_array_equal(ctx, ref[:, 0])
    np.testing.assert_array_equal(pm, pmax_of(ref[:, 0]))
    np.testing.assert_array_equal(kc2, ek)
    np.testing.assert_array_equal(vc2, vgroups(ev, kv_bs))
    np.testing.assert_array_equal(sk2, esk)
    np.testing.assert_array_equal(sv2, esv)


# ---- the division --------------------------------------------------------------------------
@pytest.mark.parametrize("H", HEADS)
def test_score_division_is_correctly_rounded(torch, H):
    """Two keys whose head-0 scores sit at 4096 and 4096 + u, u in (-3, 3): there one ulp of a
    score is 2^-11, enough to move a P code, so a product with RN(1 / c) in place of the
    division by c = fp32(sqrt(dk)) shows (asserted on the oracle: at least 4 of the 2048
    sentences); both entries must give the true-division oracle's bits on all of them."""
    rng = np.random.default_rng(H)
    B, dk = 2048, 512 // H
    c = f32(np.sqrt(dk))
    q = codes(rng, B, 1, 512)
    q[:, 0, 511] = 127                        # the row's absmax: s_q = 0.25 from y = 0.25 q
    k = np.repeat((np.sign(q) * 127).astype(np.int8), 2, axis=1)
    flip = rng.random((B, 512)) < 0.03
    k[:, 1][flip] = -k[:, 1][flip]
    acc = np.einsum("bd,bjd->bj", q[:, 0, :dk].astype(np.int64), k[:, :, :dk].astype(np.int64))
    u = rng.uniform(-3, 3, B)
    sq = np.full((B, 1), 0.25, f32)
    sk = np.stack([4096 * c / (0.25 * acc[:, 0]), (4096 + u) * c / (0.25 * acc[:, 1])], axis=1).astype(f32)
    v = rng.integers(1, 128, (B, 2, 512)).astype(np.int8) * rng.choice([-1, 1], (B, 2, 512)).astype(np.int8)
    sv = np.full((B, 2), 0.01, f32)
    ones = np.ones((B, 1, 2), np.uint8)
    ref, qp = O.attention(q, sq, k, sk, v, sv, ones, H, dec=True)
    acc4 =np.einsum("bhid,bhjd->bhij", O.split_heads(q, H).astype(np.int64), O.split_heads(k, H).astype(np.int64))
    pre = ((acc4.astype(f32) * sq[:, None, :, None]).astype(f32) * sk[:, None, None, :]).astype(f32)
    recip = (pre * (f32(1.0) / c)).astype(f32)
    differ = (O.softmax_quant(recip) != qp).any(axis=(1, 2, 3)).sum()
    print(f"H={H}: the reciprocal model changes a P code in {differ} of {B} sentences")
    assert differ >= 4
    got = run_attention(torch, H, q, sq, k, sk, v, sv, None, 0, 0, 1, POISONS[0])
    np.testing.assert_array_equal(got, ref)
    y = (q[:, 0].astype(f32) * f32(0.25)).astype(f32)
    ctx, pm, *_ = run_decode(torch, H, 0, y, k, vgroups(v, 2), sk, sv, 2, 0, 2, np.ones((B, 2), np.uint8),
                             POISONS[1])
    np.testing.assert_array_equal(ctx, ref[:, 0])
    np.testing.assert_array_equal(pm, pmax_of(ref[:, 0]))
