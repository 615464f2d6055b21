"""The decode-step kernels take their arguments as leading scalars (preloaded into SGPRs at
wave launch) plus a trailing block, packed per prologue mode at the launch sites
(csrc/qtx_decode.hip).  The failure mode of that packing is a swapped, dropped or truncated
argument, so here every argument is distinguishable — random per-channel weight scales, a
non-zero bias, LayerNorm gain != 1 and offset != 0, a residual that differs from what the
output buffer held, out == res and out != res, a row stride larger than K — and each kernel,
prologue mode and epilogue flag set of the step is compared bit for bit with the oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import qtx_oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
_KEEP = []


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def call(name, *args):
    from qtx import _lib
    _lib.call(name, *args)


# (amode, N, K): the kernel each reaches for M < 96 (qtx_decode.hip skinny_mode)
SHAPES = [
    (0, 512, 512),      # k_skinny, int8 A panel
    (0, 512, 2048),     # k_skinny K = 2048 (the step's FFN2 after the h quantizer)
    (1, 512, 512),      # k_skinny, LayerNorm prologue (LN+Qc)
    (1, 1536, 512),     # k_skinny_wide (LN+QKV)
    (1, 2048, 512),     # k_skinny_wide (LN+FFN1)
    (1, 1040, 512),     # N >= 1024 but no multiple of the wide kernel's 64 columns: k_skinny
    (2, 512, 512),      # k_skinny, partial maxima (8 heads)
    (2, 512, 2048),     # k_skinny8_ffn2<false> with the residual and 8-bit weights, else k_skinny
    (3, 512, 512),      # k_skinny, own row maximum (O / Oc: the step's dominant kernel)
    (3, 512, 2048),     # k_skinny8_ffn2<true> with the residual and 8-bit weights, else k_skinny
]
FLAGS = [0, 1, 2, 5]    # none, ReLU, residual, ReLU + row maxima
CASES = [(a, N, K, fl, 8, alias) for a, N, K in SHAPES for fl in FLAGS
         for alias in ((False, True) if fl & 2 else (False,))]
# 4-bit weights (k_skinny / k_skinny_wide only; K = 2048 then runs k_skinny with every prologue)
CASES += [(a, N, K, fl, 4, fl == 2) for a, N, K in SHAPES for fl in (2, 5)]


def _skinny_case(torch, M, amode, N, K, flags, bits, alias):
    rng = np.random.default_rng([M, amode, N, K, flags, bits, int(alias)])
    ldx = K + 8                                     # row stride > K (fp32 prologues)
    qw, sw = O.quant_weight((rng.standard_normal((N, K)) * 0.05).astype(f32), bits)
    assert np.unique(sw).size > N // 2              # per-channel scales: not constant
    b = rng.standard_normal(N).astype(f32)
    A = sa = X = lna = lnb = pin = None
    nparts = 0
    if amode == 0:
        qx, sx = O.quant_rows(rng.standard_normal((M, K)).astype(f32))
        A, sa = dev(torch, qx), dev(torch, sx)
    else:
        x = (rng.standard_normal((M, K)) * 3).astype(f32)
        if amode != 1 and K == 2048:
            x = np.maximum(x, 0)                    # a ReLU hidden
        xp = np.full((M, ldx), np.nan, f32)         # the stride's gap is never read
        xp[:, :K] = x
        X = dev(torch, xp)
        if amode == 1:
            a = rng.uniform(0.5, 1.5, K).astype(f32)
            bb = rng.uniform(-0.5, 0.5, K).astype(f32)
            lna, lnb = dev(torch, a), dev(torch, bb)
            qx, sx = O.quant_rows(O.layer_norm(x, a, bb))
        else:
            qx, sx = O.quant_rows(x)
        if amode == 2:
            nparts = 8 if K == 512 else 128
            pin = dev(torch, np.abs(x).reshape(M, nparts, K // nparts).max(-1).T.copy())
    res = rng.standard_normal((M, N)).astype(f32)
    # out != res: the output buffer starts as NaN, so a residual read from it shows
    out = dev(torch, res.copy() if alias else np.full((M, N), np.nan, f32))
    resd = out if alias else (dev(torch, res) if flags & 2 else None)
    pm = dev(torch, np.full((N // 16, M), np.nan, f32)) if flags & 4 else None
    wd = dev(torch, qw)
    if bits == 4:
        packed = torch.empty((N, K // 2), dtype=torch.uint8, device="cuda")
        call("qtx_pack_int4", P(wd), N, K, P(packed), S0)
        _KEEP.append(packed)
        wd = packed
    call("qtx_skinny_linear", amode, P(A), P(sa), P(X), ldx if amode else 0, P(lna), P(lnb),
         P(pin), nparts, P(wd), P(dev(torch, sw)), P(dev(torch, b)), M, N, K, bits, flags,
         P(resd), P(out), P(pm), S0)
    y = O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b, relu=bool(flags & 1))
    if flags & 2:
        y = res + y
    np.testing.assert_array_equal(out.cpu().numpy(), y)
    if flags & 4:
        np.testing.assert_array_equal(pm.cpu().numpy(),
                                      np.abs(y).reshape(M, N // 16, 16).max(-1).T)
    if flags & 2 and not alias:
        np.testing.assert_array_equal(resd.cpu().numpy(), res)      # the residual is only read


@pytest.mark.parametrize("M", [1, 4, 5, 33])   # below a row block, exact, ragged, > one MFMA row tile
@pytest.mark.parametrize("amode,N,K,flags,bits,alias", CASES)
def test_skinny_arguments(torch, M, amode, N, K, flags, bits, alias):
    _skinny_case(torch, M, amode, N, K, flags, bits, alias)


@pytest.mark.parametrize("amode,N,K,flags", [(1, 1536, 512, 0), (3, 512, 512, 2), (1, 2048, 512, 1),
                                             (0, 512, 2048, 2), (3, 512, 2048, 2)])
def test_skinny_arguments_large_batch(torch, amode, N, K, flags):
    """From 96 rows the step runs other instantiations (8-row N-split blocks for K = 512,
    16-row / 8-row blocks for K = 2048): 97 rows, the last block ragged."""
    _skinny_case(torch, 97, amode, N, K, flags, 8, False)


def vgroup4(v):
    """[B, n, 512] int8 values -> qtx_decode_attention's 4-key group layout
    [B, ceil(n/4), 512, 4] (include/qtx.h)."""
    B, n, D = v.shape
    g4 = (n + 3) // 4
    vp = np.zeros((B, 4 * g4, D), np.int8)
    vp[:, :n] = v
    return np.ascontiguousarray(vp.reshape(B, g4, 4, D).transpose(0, 1, 3, 2))


def vungroup4(vg, n):
    B, g4, D, _ = vg.shape
    return vg.transpose(0, 1, 3, 2).reshape(B, 4 * g4, D)[:, :n]


def head_max(ctx):
    return np.abs(ctx).reshape(-1, 8, 64).max(-1).T


def _caches(rng, B, n):
    return (rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.uniform(0.002, 0.03, (B, n)).astype(f32),
            rng.uniform(0.002, 0.03, (B, n)).astype(f32))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("keys,kv_bs", [(1, 6), (4, 6), (5, 6), (5, 74), (72, 74)])
def test_decode_self_attention_arguments(torch, B, keys, kv_bs):
    """Self-attention with the position read from the device counter (the only form the C-ABI
    entry has; the host-position form runs in test_tiny_greedy_decode's default graph): keys
    0 .. keys - 1 of a cache of kv_bs rows (no multiple of the value layout's 4-key groups),
    y rows 8 floats apart from dense.  The new k / v row lands at row keys - 1 of its
    sentence and nothing else in the caches changes."""
    rng = np.random.default_rng([B, keys, kv_bs])
    step, ldy = keys - 1, 1536 + 8
    y = np.full((B, ldy), np.nan, f32)
    y[:, :1536] = rng.standard_normal((B, 1536)) * np.array([1.0, 2.0, 0.5]).repeat(512)
    kc, vc, skc, svc = _caches(rng, B, kv_bs)
    kcd, vcd, skd, svd = dev(torch, kc), dev(torch, vgroup4(vc)), dev(torch, skc), dev(torch, svc)
    stepd = dev(torch, np.array([step], np.int32))
    ctxd = dev(torch, np.full((B, 512), np.nan, f32))
    pm = dev(torch, np.full((8, B), np.nan, f32))
    call("qtx_decode_attention", 1, P(dev(torch, y)), ldy, P(kcd), P(vcd), P(skd), P(svd), kv_bs,
         P(stepd), 0, S0, B, P(ctxd), P(pm), S0)
    qq, sq = O.quant_rows(y[:, :512])
    qk, sk = O.quant_rows(y[:, 512:1024])
    qv, sv = O.quant_rows(y[:, 1024:1536])
    kc[:, step], vc[:, step], skc[:, step], svc[:, step] = qk, qv, sk, sv
    np.testing.assert_array_equal(kcd.cpu().numpy(), kc)
    np.testing.assert_array_equal(vungroup4(vcd.cpu().numpy(), kv_bs), vc)
    np.testing.assert_array_equal(skd.cpu().numpy(), skc)
    np.testing.assert_array_equal(svd.cpu().numpy(), svc)
    assert stepd.cpu().tolist() == [step]
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc[:, :keys], skc[:, :keys], vc[:, :keys],
                         svc[:, :keys], np.ones((B, 1, keys), np.uint8), dec=True)
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 4, 5, 72])
def test_decode_cross_attention_arguments(torch, B, S):
    """Cross-attention over S keys of caches whose sentences are kv_bs > S rows apart (no
    multiple of 4): a masked tail in sentence 0, sentence 1 fully masked (the uniform softmax
    over all S keys), sentence 2 unmasked."""
    rng = np.random.default_rng([B, S])
    kv_bs = S + 1 if (S + 1) % 4 else S + 2
    ldy = 512 + 8
    y = np.full((B, ldy), np.nan, f32)
    y[:, :512] = rng.standard_normal((B, 512))
    kc, vc, skc, svc = _caches(rng, B, kv_bs)
    mask = np.ones((B, S), np.uint8)
    mask[0, (S + 1) // 2:] = 0                      # (S = 1: nothing to mask)
    if B > 1:
        mask[1, :] = 0
    ctxd = dev(torch, np.full((B, 512), np.nan, f32))
    pm = dev(torch, np.full((8, B), np.nan, f32))
    call("qtx_decode_attention", 0, P(dev(torch, y)), ldy, P(dev(torch, kc)),
         P(dev(torch, vgroup4(vc))), P(dev(torch, skc)), P(dev(torch, svc)), kv_bs, S0, S,
         P(dev(torch, mask)), B, P(ctxd), P(pm), S0)
    qq, sq = O.quant_rows(y[:, :512])
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc[:, :S], skc[:, :S], vc[:, :S], svc[:, :S],
                         mask[:, None], dec=True)
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


@pytest.fixture(scope="module")
def tiny_decode(oracle_model):
    rng = np.random.default_rng(11)
    src = np.full((3, 8), 2, np.int64)
    for b, n in enumerate([8, 5, 3]):
        src[b, 0] = 0
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        src[b, n - 1] = 1
    mask = (src != 2)[:, None, :]
    return src, mask, oracle_model.greedy_decode(src, mask, 6)


@pytest.mark.parametrize("env", [{}, {"QTX_GRAPH_STEPS": "1"}], ids=["default", "graph_steps_1"])
def test_tiny_greedy_decode(torch, gpu_model, knob_env, tiny_decode, env):
    """B = 3, S = 8, max_len = 6 against the oracle's ids: the default decode (every step
    captured at its own position: the host-position form of the attention and of the tail),
    and one captured step replayed at the 5 positions (the device-counter form)."""
    from qtx.decode import greedy_decode
    src, mask, ref = tiny_decode
    for k, v in env.items():
        knob_env(k, v)
    np.testing.assert_array_equal(greedy_decode(gpu_model, src, mask, 6, 0), ref)
