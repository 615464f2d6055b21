"""The fused decode step past 128 keys: k_dec_attn_long (csrc/qtx_decode_long.hip) through
qtx_decode_attention at 129 to 512 keys, and the plain / scored greedy decode on the fused step
and its graphs at max_len = 140 and S = 132 — against the oracle, bit for bit.

The key counts are the kernel's edges: 129 (one key in the second wave's block and the third
lane round), 257 (one key in the third wave's block), 511 / 512 (the ragged and the full last
round); the self-attention steps put the new key first and last in a wave's block.  Random
caches give most keys P == 0, so test_cross_one_hot and test_self_every_step put P == 127 on
one key slot after the other and on every step's patch of the new key, value byte and scales."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_attn as LA  # noqa: E402
import long_target as LT  # noqa: E402
from guarded import guarded  # noqa: E402
from test_gpu_fused import P, S0, _release, call, dev, head_max, torch, vgroup4  # noqa: E402,F401
from test_gpu_scored import gpu_scored  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
B = 3


def caches(rng, n):
    return (rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.uniform(0.002, 0.03, (B, n)).astype(f32), rng.uniform(0.002, 0.03, (B, n)).astype(f32))


def filled(torch, a, name):
    """`a` on the device between guard bands: (tensor, check)."""
    t, chk = guarded(torch, a.shape, getattr(torch, str(a.dtype)), 0x5A, name=name)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t, chk


@pytest.mark.parametrize("third", ["masked", "one_key"])
@pytest.mark.parametrize("S", [129, 192, 257, 511, 512])
def test_cross_attention(torch, S, third):
    """Sentence 0 loses its last third, sentence 1 every seventh key, sentence 2 is fully masked
    (the uniform softmax over all S keys) or keeps one key in the last lane round (P = 127
    there: a softmax that drops a lane round, or a PV chain that stops short, loses it)."""
    rng = np.random.default_rng(4000 + S)
    y = rng.standard_normal((B, 512)).astype(f32)
    kc, vc, skc, svc = caches(rng, S)
    mask = np.ones((B, S), np.uint8)
    mask[0, S - S // 3:] = 0
    mask[1, 1::7] = 0
    mask[2] = 0
    j = 64 * ((S - 1) // 64)
    if third == "one_key":
        mask[2, j] = 1
    qq, sq = O.quant_rows(y)
    ctx, qp = O.attention(qq[:, None], sq[:, None], kc, skc, vc, svc, mask[:, None], dec=True)
    if third == "one_key":
        assert (qp[2, :, 0, j] == 127).all() and (qp[2, :, 0].astype(np.int64).sum(-1) == 127).all()
    ctxd, c0 = guarded(torch, (B, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, B), torch.float32, 0x5A, name="pmax")
    call("qtx_decode_attention", 0, P(dev(torch, y)), 512, P(dev(torch, kc)), P(dev(torch, vgroup4(vc))),
         P(dev(torch, skc)), P(dev(torch, svc)), S, S0, S, P(dev(torch, mask)), B, P(ctxd), P(pm), S0)
    torch.cuda.synchronize()
    c0()
    c1()
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


@pytest.mark.parametrize("step,kv_bs", [(s, 512) for s in (128, 129, 255, 256, 383, 511)] + [(139, 140)])
def test_self_attention(torch, step, kv_bs):
    """The position from the device counter; the cached row at `step` holds other codes and
    scales, which must not reach the result; the append changes row `step` alone (whole
    buffers compared, guard bands checked)."""
    rng = np.random.default_rng(6000 + step)
    y = rng.standard_normal((B, 1536)).astype(f32)
    kc, vc, skc, svc = caches(rng, kv_bs)
    bufs = [filled(torch, a, n) for a, n in ((kc, "kc"), (vgroup4(vc), "vc"), (skc, "skc"), (svc, "svc"))]
    (kcd, vcd, skd, svd), checks = zip(*bufs)
    ctxd, c0 = guarded(torch, (B, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, B), torch.float32, 0x5A, name="pmax")
    qq, sq = O.quant_rows(y[:, :512])
    kc[:, step], skc[:, step] = O.quant_rows(y[:, 512:1024])
    vc[:, step], svc[:, step] = O.quant_rows(y[:, 1024:])
    n = step + 1
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc[:, :n], skc[:, :n], vc[:, :n], svc[:, :n],
                         np.ones((B, 1, n), np.uint8), dec=True)
    call("qtx_decode_attention", 1, P(dev(torch, y)), 1536, P(kcd), P(vcd), P(skd), P(svd), kv_bs,
         P(dev(torch, np.array([step], np.int32))), 0, S0, B, P(ctxd), P(pm), S0)
    torch.cuda.synchronize()
    for chk in checks + (c0, c1):
        chk()
    for got, want in ((kcd, kc), (vcd, vgroup4(vc)), (skd, skc), (svd, svc), (ctxd, ctx[:, 0]),
                      (pm, head_max(ctx[:, 0]))):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- every key slot and every step, directed (tests/long_attn.py) ----------------------------
@pytest.mark.parametrize("S", [129, 511, 512])
def test_cross_one_hot(torch, S):
    """B = S sentences in one launch, sentence b keeps key b alone: P == 127 / 127 on one key
    slot after the other, random nonzero values and scales everywhere.  The context is that
    key's value row times its scale, so a wrong value byte, group dword, clamp or scale of any
    one slot fails its sentence."""
    c = LA.one_hot(S)
    qq, sq = O.quant_rows(c["y"])
    ctx, qp = LA.attention_chunked(qq, sq, c["kc"], c["skc"], c["vc"], c["svc"], c["mask"])
    np.testing.assert_array_equal(qp, np.repeat((127 * np.eye(S, dtype=np.int8))[:, None], 8, 1))
    np.testing.assert_array_equal(ctx, c["ctx"])        # RN(RN(1 * s_v[b, b]) * v[b, b, :])
    ctxd, c0 = guarded(torch, (S, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, S), torch.float32, 0x5A, name="pmax")
    call("qtx_decode_attention", 0, P(dev(torch, c["y"])), 512, P(dev(torch, c["kc"])),
         P(dev(torch, vgroup4(c["vc"]))), P(dev(torch, c["skc"])), P(dev(torch, c["svc"])), S, S0, S,
         P(dev(torch, c["mask"])), S, P(ctxd), P(pm), S0)
    torch.cuda.synchronize()
    c0()
    c1()
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx)
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx))


def test_self_every_step(torch):
    """The steps 0 .. 511 at kv_bs = 512 (the dispatch is by kv_bs, so the steps below 128 run
    k_dec_attn_long too), the position from the device counter, on one pair of caches.
    Sentence 0: the new key is the only live one; sentence 1: a cached key that walks the slots,
    the new key dead.  Row `step` holds stale codes and scales before the call.  After every
    step the context, the head maxima and the whole caches are compared (on the device: the
    caches before the call with row `step` replaced by the closed form's), the guard bands once
    at the end."""
    es = LA.EveryStep()
    n = LA.KV_BS
    rng = np.random.default_rng(9001)
    kc = np.repeat(es.dead[:, None], n, 1)                       # every cached key dead
    vc = rng.integers(-127, 128, (2, n, 512)).astype(np.int8)
    skc, svc = np.full((2, n), LA.SK_DEAD, f32), rng.uniform(0.002, 0.03, (2, n)).astype(f32)
    bufs = [filled(torch, a, nm) for a, nm in ((kc, "kc"), (vgroup4(vc), "vc"), (skc, "skc"), (svc, "svc"))]
    (kcd, vcd, skd, svd), checks = zip(*bufs)
    ctxd, c0 = guarded(torch, (2, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, 2), torch.float32, 0x5A, name="pmax")
    yd, steps = dev(torch, es.y), dev(torch, np.arange(n, dtype=np.int32))
    qk, qv, sk, sv = (dev(torch, a) for a in (es.qk, es.qv, es.sk, es.sv))
    stale_v = dev(torch, es.stale_v)
    ctx_want = dev(torch, es.ctx)
    pm_want = dev(torch, np.stack([head_max(c) for c in es.ctx]))
    bad = []
    for step in range(n):
        for b, r, k_row, k_scale in es.before(step):
            kcd[b, r].copy_(torch.from_numpy(np.array(k_row)))
            skd[b, r] = float(k_scale)
        vcd[:, step >> 2, :, step & 3] = stale_v[step]
        svd[:, step] = float(LA.SV_STALE)
        want = [t.clone() for t in (kcd, vcd, skd, svd)]
        want[0][:, step], want[1][:, step >> 2, :, step & 3] = qk[step], qv[step]
        want[2][:, step], want[3][:, step] = sk[step], sv[step]
        call("qtx_decode_attention", 1, P(yd[step]), 1536, P(kcd), P(vcd), P(skd), P(svd), n,
             C.c_void_p(steps.data_ptr() + 4 * step), 0, S0, 2, P(ctxd), P(pm), S0)
        ok = [torch.equal(g, w) for g, w in zip((kcd, vcd, skd, svd), want)]
        ok += [torch.equal(ctxd, ctx_want[step]), torch.equal(pm, pm_want[step])]
        if not all(ok):
            bad.append((step, ok))
    torch.cuda.synchronize()
    for chk in checks + (c0, c1):
        chk()
    assert not bad, f"{len(bad)} steps differ (kc, vc, skc, svc, ctx, pmax): {bad[:8]}"


# ---- model level: the fused-capable models of the long-target regime ------------------------
MODELS = [(512, 8), (512, 4)]


def fresh(c):
    from qtx.model import QtxModel
    cfg, sd, _ = LT.state(*c)
    gm = QtxModel(sd, cfg)
    gm.workspace(64 << 20)        # sized once: every call carves the same memory
    return gm


def stats(gm):
    """(entries, captures) of the model's graph cache."""
    import ctypes as C
    e, n = C.c_int32(-1), C.c_int64(-1)
    call("qtx_debug_graph_stats", gm.handle, C.byref(e), C.byref(n))
    return e.value, n.value


def long_greedy(c):
    """The oracle's greedy decode of LT.long_inputs() to L (its prefixes: the shorter decodes)."""
    src, m = LT.long_inputs()
    return LT.memo(("long_greedy", c), lambda: LT.state(*c)[2].greedy_decode(src, m, LT.L))


@pytest.mark.parametrize("c", MODELS, ids=LT.cfg_id)
def test_decode_is_captured(torch, c):
    """L = 140 runs on graphs of the fused step: at least one capture by the first call, none
    by the second."""
    gm = fresh(c)
    src, m = LT.inputs()
    srcd, md = dev(torch, src), dev(torch, m.reshape(LT.B, LT.S).astype(np.uint8))
    assert stats(gm) == (0, 0)
    seen = []
    for _ in range(2):
        ids = gm.greedy(srcd, md, LT.L, 0)
        np.testing.assert_array_equal(ids.cpu().numpy(), LT.scored(c)[0])
        seen.append(stats(gm))
    assert seen[0][1] >= 1 and seen[1] == seen[0], seen


@pytest.mark.parametrize("env,L", [({}, LT.L), ({"QTX_NO_GRAPH": 1}, LT.L), ({"QTX_GRAPH_STEPS": 8}, 137),
                                   ({"QTX_UNFUSED": 1}, LT.L)],
                         ids=["default", "no_graph", "graph_steps_8", "unfused"])
@pytest.mark.parametrize("c", MODELS, ids=LT.cfg_id)
def test_greedy_and_scored(torch, knob_env, c, env, L):
    """ids / top_ids / top_logp at L (a decode to a shorter max_len is a prefix of the longer
    one; 137 = 136 steps in graphs of 8 at the device counter, past 128), and the S = 132 source
    with a short (12) and a long target."""
    from qtx.decode import greedy_decode
    for k, v in env.items():
        knob_env(k, v)
    gm = fresh(c)
    src, m = LT.inputs()
    oy, oi, ov = LT.scored(c)
    gy, gi, gv = gpu_scored(gm, src, m, L)
    np.testing.assert_array_equal(gy, oy[:, :L])
    np.testing.assert_array_equal(gi, oi[:, :L - 1])
    np.testing.assert_array_equal(gv, ov[:, :L - 1])
    np.testing.assert_array_equal(greedy_decode(gm, src, m, L, 0), oy[:, :L])
    src, m = LT.long_inputs()
    for n in (12, L):
        np.testing.assert_array_equal(greedy_decode(gm, src, m, n, 0), long_greedy(c)[:, :n])


@pytest.mark.parametrize("long_src,L", [(True, 12), (False, LT.L)], ids=["S132", "L140"])
def test_enctrials_stays_unfused_past_128(torch, long_src, L):
    """The encoder trials decode shares greedy_steps but keeps the 128-key rule: its prologue
    regroups no cross values past 128, so its steps must be the unfused ones.  All rows golden:
    the plain decode's ids."""
    from qtx.decode import greedy_decode_enctrials
    c = MODELS[0]
    src, m = LT.long_inputs() if long_src else LT.inputs()
    want = long_greedy(c)[:, :L] if long_src else LT.scored(c)[0]
    ys, _ = greedy_decode_enctrials(fresh(c), src, m, L, 0, [None] * src.shape[0])
    np.testing.assert_array_equal(ys, want)
