"""The fused decode step past 128 keys: k_dec_attn_long (csrc/qtx_decode_long.hip) through
qtx_decode_attention at 129 to 512 keys, and the plain / scored greedy decode on the fused step
and its graphs at max_len = 140 and S = 132 — against the oracle, bit for bit.

The key counts are the kernel's edges: 129 (one key in the second wave's block and the third
lane round), 257 (one key in the third wave's block), 511 / 512 (the ragged and the full last
round); the self-attention steps put the new key first and last in a wave's block."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
