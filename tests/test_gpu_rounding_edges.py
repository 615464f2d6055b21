"""Every per-token quantizer of the library on rounding ties and their floating-point
neighbours (tests/rounding_edges.py), bit-exact against the oracle's rint(x / s).

The rows reach each quantizer as they are (fp32 inputs), through a LayerNorm with gamma = 0
and beta = the tie row (LN(x) == beta bit for bit), or through a GEMM epilogue whose output
rows are tie rows times a power of two (one-hot codes, sw = the tie row).  That these inputs
would fail a quantizer that drops its near-tie fallback, loses div_cr's correction step or
rounds half away from zero is shown on the CPU by tests/test_rounding_edges_ref.py.  Codes,
scales and downstream floats are all compared with assert_array_equal.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounding_edges as E  # noqa: E402
from test_gpu_fused import head_max, vgroup4, vungroup4  # noqa: E402
from test_gpu_ops import P, S0, _from_kp, _release, _rows_call, _to_kp, call, torch  # noqa: E402,F401
from test_gpu_ops import dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ZEROS = np.zeros(512, f32)


def dev(torch, a):
    """test_gpu_ops.dev on a private copy (the generator's arrays are read-only)."""
    return _dev(torch, np.array(a))


def empty(torch, shape, dtype):
    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")


def zeros(torch, shape, dtype):
    return torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")


def pack_w(torch, qw, kp):
    """W as qtx_linear_rows reads it with this kp: row-major, KP, or weight-stationary."""
    from qtx._lib import lib
    wd = dev(torch, qw)
    if kp == 0:
        return wd
    out = empty(torch, qw.shape, "int8")
    fn = lib().qtx_pack_w_kp if kp == 1 else lib().qtx_pack_w_ws
    assert fn(P(wd), qw.shape[0], qw.shape[1], P(out), S0) == 0
    return out


# ----------------------------------------------------------------- direct fp32 input
@pytest.mark.parametrize("D", [256, 512, 768, 2048])
def test_row_quant(torch, D):
    """k_rows / quant_pack<N> on every row of every (mantissa, exponent) set, with qmax 127 and
    with qmax 7 (the int4 weight quantizer, ties k + 1/2 for |k| <= 6); with qmax 127 also the
    lone rows (one near-tie per row, at every slot of a lane: the wave vote must see it)."""
    for qmax, bits in ((127.0, 8), (7.0, 4)):
        x = E.all_rows(D, qmax)
        if bits == 8:
            x = np.concatenate([x, E.lone_rows(D)[0]])
        q = empty(torch, x.shape, "int8")
        s = empty(torch, (len(x),), "float32")
        call("qtx_row_quant", P(dev(torch, x)), len(x), D, qmax, P(q), P(s), S0)
        qo, so = O.quant_rows(x, bits)
        np.testing.assert_array_equal(s.cpu().numpy(), so)
        np.testing.assert_array_equal(q.cpu().numpy(), qo)


@pytest.mark.parametrize("amode,K,nparts,M,start", E.SKINNY_DIRECT)
def test_skinny_prologue(torch, amode, K, nparts, M, start):
    """The skinny GEMM's fp32 prologues: amode 3 (own row maximum) and amode 2 (complete
    partial maxima); M = 3 runs k_skinny8_ffn2 at K = 2048, 40 k_skinny, 100 the 8-row blocks
    and k_skinny_wide.  Tie rows and lone rows alternate.  Random int8 W: one wrong code
    changes the whole output row."""
    rng = np.random.default_rng(1000 * amode + K + nparts + M)
    h, _ = E.direct_rows(K, M, start)
    qw, sw, b = E.rand_weights(rng, 512, K)
    res = rng.standard_normal((M, 512)).astype(f32)
    out = dev(torch, res.copy())
    parts = S0
    if amode == 2:
        parts = P(dev(torch, np.abs(h).reshape(M, nparts, K // nparts).max(-1).T.copy()))
    call("qtx_skinny_linear", amode, S0, S0, P(dev(torch, h)), K, S0, S0, parts, nparts,
         P(dev(torch, qw)), P(dev(torch, sw)), P(dev(torch, b)), M, 512, K, 8, 2,
         P(out), P(out), S0, S0)
    qx, sx = O.quant_rows(h)
    np.testing.assert_array_equal(out.cpu().numpy(),
                                  res + O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b))


@pytest.mark.parametrize("lone", [False, True])
def test_decode_self_attention(torch, lone):
    """quant_one on the step's q | k | v thirds (three mantissas per sentence; tie rows, or
    lone rows: one near-tie in one lane of the wave): the appended cache row's codes and
    scales directly, and the context and head maxima that depend on q's codes."""
    B, step, kv_bs = 3, 5, 8
    rng = np.random.default_rng(17)
    y = E.decode_y(B, lone=lone)
    kc = rng.integers(-127, 128, (B, kv_bs, 512)).astype(np.int8)
    vc = rng.integers(-127, 128, (B, kv_bs, 512)).astype(np.int8)
    skc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
    svc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
    kcd, vcd, skd, svd = dev(torch, kc), dev(torch, vgroup4(vc)), dev(torch, skc), dev(torch, svc)
    ctxd = empty(torch, (B, 512), "float32")
    pm = empty(torch, (8, B), "float32")
    call("qtx_decode_attention", 1, P(dev(torch, y)), 1536, P(kcd), P(vcd), P(skd), P(svd),
         kv_bs, P(dev(torch, np.array([step], np.int32))), 0, S0, B, P(ctxd), P(pm), S0)
    qq, sq = O.quant_rows(y[:, :512])
    qk, sk = O.quant_rows(y[:, 512:1024])
    qv, sv = O.quant_rows(y[:, 1024:])
    np.testing.assert_array_equal(kcd.cpu().numpy()[:, step], qk)
    np.testing.assert_array_equal(vungroup4(vcd.cpu().numpy(), kv_bs)[:, step], qv)
    np.testing.assert_array_equal(skd.cpu().numpy()[:, step], sk)
    np.testing.assert_array_equal(svd.cpu().numpy()[:, step], sv)
    kc[:, step], vc[:, step], skc[:, step], svc[:, step] = qk, qv, sk, sv
    np.testing.assert_array_equal(kcd.cpu().numpy(), kc)
    np.testing.assert_array_equal(vungroup4(vcd.cpu().numpy(), kv_bs), vc)
    n = step + 1
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc[:, :n], skc[:, :n], vc[:, :n],
                         svc[:, :n], np.ones((B, 1, n), np.uint8), dec=True)
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


def test_decode_cross_attention(torch):
    """quant_one on tie rows and lone rows as the cross attention's q (kv_new = 0), S = 17."""
    S = 17
    rng = np.random.default_rng(23)
    y = E.direct_rows(*E.DECODE_CROSS_Q)[0]
    B = len(y)
    kc = rng.integers(-127, 128, (B, S, 512)).astype(np.int8)
    vc = rng.integers(-127, 128, (B, S, 512)).astype(np.int8)
    skc = rng.uniform(0.002, 0.03, (B, S)).astype(f32)
    svc = rng.uniform(0.002, 0.03, (B, S)).astype(f32)
    mask = np.ones((B, S), np.uint8)
    mask[1, 11:] = 0
    ctxd = empty(torch, (B, 512), "float32")
    pm = empty(torch, (8, B), "float32")
    call("qtx_decode_attention", 0, P(dev(torch, y)), 512, P(dev(torch, kc)),
         P(dev(torch, vgroup4(vc))), P(dev(torch, skc)), P(dev(torch, svc)), S, S0, S,
         P(dev(torch, mask)), B, P(ctxd), P(pm), S0)
    qq, sq = O.quant_rows(y)
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc, skc, vc, svc, mask[:, None], dec=True)
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


# ----------------------------------------------------------------- through a LayerNorm
def test_layernorm_quant(torch):
    """k_rows in LayerNorm mode: gamma = 0, beta = each of the 18 tie rows and 24 lone rows."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((7, 512)) * 3).astype(f32)
    xd, ad = dev(torch, x), dev(torch, ZEROS)
    y, q = empty(torch, x.shape, "float32"), empty(torch, x.shape, "int8")
    s = empty(torch, (7,), "float32")
    for beta in E.betas():
        call("qtx_layernorm_quant", P(xd), P(ad), P(dev(torch, beta)), 7, 512, P(y), P(q), P(s), S0)
        yo = O.layer_norm(x, ZEROS, beta)
        np.testing.assert_array_equal(y.cpu().numpy(), yo)
        qo, so = O.quant_rows(yo)
        np.testing.assert_array_equal(s.cpu().numpy(), so)
        np.testing.assert_array_equal(q.cpu().numpy(), qo)


@pytest.mark.parametrize("M", [5, 32, 98])
@pytest.mark.parametrize("N", [1536, 2048])
def test_skinny_layernorm_prologue(torch, N, M):
    """amode 1 (quant_rows512 behind the LayerNorm of k_skinny_wide / k_skinny): N = 1536 plain,
    N = 2048 with ReLU and the output's tile maxima."""
    rng = np.random.default_rng(N + M)
    x = (rng.standard_normal((M, 512)) * 3).astype(f32)
    qw, sw, b = E.rand_weights(rng, N, 512)
    relu = N == 2048
    xd, ad, wd, swd, bd = (dev(torch, a) for a in (x, ZEROS, qw, sw, b))
    out = empty(torch, (M, N), "float32")
    pm = zeros(torch, (N // 16, M), "float32")
    for beta in E.betas():
        call("qtx_skinny_linear", 1, S0, S0, P(xd), 512, P(ad), P(dev(torch, beta)), S0, 0,
             P(wd), P(swd), P(bd), M, N, 512, 8, (1 | 4) if relu else 0, S0, P(out),
             P(pm) if relu else S0, S0)
        qx, sx = O.quant_rows(O.layer_norm(x, ZEROS, beta))
        y = O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b, relu=relu)
        np.testing.assert_array_equal(out.cpu().numpy(), y)
        if relu:
            np.testing.assert_array_equal(pm.cpu().numpy(),
                                          np.abs(y).reshape(M, N // 16, 16).max(-1).T)


@pytest.mark.parametrize("kp,M,K,ksplit", [(0, 37, 512, 0), (1, 130, 512, 0), (1, 7, 2048, 4),
                                           (2, 97, 512, 0)])
def test_linear_rows_residual_layernorm(torch, kp, M, K, ksplit):
    """epi 1 with lnq: the row-major kernel, the KP kernel, its split-K epilogue
    (k_res_ln_partials) and the weight-stationary kernel."""
    rng = np.random.default_rng(100 * kp + M + K)
    qx, sx = O.quant_rows(rng.standard_normal((M, K)).astype(f32))
    qw, sw = O.quant_weight((rng.standard_normal((512, K)) * 0.05).astype(f32), 8)
    b = rng.standard_normal(512).astype(f32)
    res = (rng.standard_normal((M, 512)) * 2).astype(f32)
    x = res + O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b)
    Mp = M + (M & 1) if kp else M
    lnq, lns = zeros(torch, (Mp, 512), "int8"), empty(torch, (M,), "float32")
    kw = dict(A=dev(torch, _to_kp(qx) if kp else qx), sa=dev(torch, sx), W=pack_w(torch, qw, kp),
              sw=dev(torch, sw), bias=dev(torch, b), M=M, N=512, K=K, epi=1,
              ln_a=dev(torch, ZEROS), lnq=lnq, lns=lns, kp=kp)
    if ksplit:
        kw.update(part=empty(torch, (ksplit * M * 512,), "int32"), ksplit=ksplit)
    for beta in E.betas():
        xd = dev(torch, res.copy())
        _rows_call(torch, res=xd, xout=xd, ln_b=dev(torch, beta), **kw)
        np.testing.assert_array_equal(xd.cpu().numpy(), x)
        q, s = O.quant_rows(O.layer_norm(x, ZEROS, beta))
        got = lnq.cpu().numpy()
        np.testing.assert_array_equal(lns.cpu().numpy(), s)
        np.testing.assert_array_equal(_from_kp(got, M) if kp else got, q)


class Ffn:
    """One qtx_ffn_rows problem (M rows, d_ff F): random by default, any piece replaceable;
    run() calls the kernel, oracle() restates it."""

    def __init__(self, torch, M, F, seed):
        from test_gpu_ffn import to_kp
        rng = np.random.default_rng(seed + M + F)
        self.torch, self.M, self.F, self.to_kp = torch, M, F, to_kp
        self.x1 = (rng.standard_normal((M, 512)) * 2).astype(f32)
        self.qx, self.sx = O.quant_rows(rng.standard_normal((M, 512)).astype(f32))
        self.qw1, self.sw1 = O.quant_weight((rng.standard_normal((F, 512)) * 0.05).astype(f32), 8)
        self.qw2, self.sw2 = O.quant_weight((rng.standard_normal((512, F)) * 0.05).astype(f32), 8)
        self.b1 = (rng.standard_normal(F) * 0.1).astype(f32)
        self.b2 = (rng.standard_normal(512) * 0.1).astype(f32)
        self.na = (1 + 0.1 * rng.standard_normal(512)).astype(f32)
        self.nb = (0.1 * rng.standard_normal(512)).astype(f32)

    def run(self):
        from qtx._lib import FfnRows, lib
        from test_gpu_ffn import from_kp
        torch, M, F = self.torch, self.M, self.F
        wf = empty(torch, (F * 1024,), "int8")
        assert lib().qtx_pack_ffn(P(dev(torch, self.qw1)), P(dev(torch, self.qw2)), F, P(wf), S0) == 0
        x = dev(torch, self.x1.copy())
        q8, qs = zeros(torch, (M + (M & 1), 512), "int8"), empty(torch, (M,), "float32")
        a = FfnRows()
        a.A, a.sa = dev(torch, self.to_kp(self.qx)).data_ptr(), dev(torch, self.sx).data_ptr()
        a.wf = wf.data_ptr()
        a.sw1, a.b1 = dev(torch, self.sw1).data_ptr(), dev(torch, self.b1).data_ptr()
        a.sw2, a.b2 = dev(torch, self.sw2).data_ptr(), dev(torch, self.b2).data_ptr()
        a.ln_a, a.ln_b = dev(torch, self.na).data_ptr(), dev(torch, self.nb).data_ptr()
        a.x = x.data_ptr()
        a.lnq, a.lns, a.M, a.F = q8.data_ptr(), qs.data_ptr(), M, F
        rc = lib().qtx_ffn_rows(C.byref(a), S0)
        assert rc == 0, lib().qtx_last_error()
        torch.cuda.synchronize()
        return x.cpu().numpy(), from_kp(q8.cpu().numpy(), M), qs.cpu().numpy()

    def oracle_x(self):
        h = O.linear_epilogue(O.int_gemm(self.qx, self.qw1), self.sx, self.sw1, self.b1, relu=True)
        qh, sh = O.quant_rows(h)
        return self.x1 + O.linear_epilogue(O.int_gemm(qh, self.qw2), sh, self.sw2, self.b2)

    def check(self, x2):
        x, q, s = self.run()
        np.testing.assert_array_equal(x, x2)
        qo, so = O.quant_rows(O.layer_norm(x2, self.na, self.nb))
        np.testing.assert_array_equal(s, so)
        np.testing.assert_array_equal(q, qo)


@pytest.mark.parametrize("F", [256, 2048])
def test_ffn_rows_final_quantizer(torch, F):
    """k_ffn_fused's LayerNorm quantizer: gamma = 0, beta = each tie row, M = 130."""
    f = Ffn(torch, 130, F, 1)
    f.na = ZEROS
    x2 = f.oracle_x()
    for beta in E.betas():
        f.nb = beta
        f.check(x2)


@pytest.mark.parametrize("F", [256, 2048])
def test_ffn_rows_hidden_quantizer(torch, F):
    """k_ffn_fused's hidden quantizer: A = 0, so h = relu(b1) with b1 the F-wide tie row; a
    wrong hidden code changes x through the random W2."""
    f = Ffn(torch, 130, F, 2)
    f.qx = np.zeros_like(f.qx)
    for st in E.FFN_HIDDEN_STARTS:
        f.b1 = E.ffn_hidden_bias(F, st)
        f.check(f.oracle_x())


# ----------------------------------------------------------------- through a GEMM epilogue
@pytest.mark.parametrize("M", [97, 300])
@pytest.mark.parametrize("kp", [0, 1, 2])
def test_linear_rows_qkv(torch, kp, M):
    """epi 0 (k_gemm_row, its KP form, k_gemm_wsq and its tail): each 512-column tile of y is a
    tie row of a different set times 2**(m % 5 - 2), a lone row likewise, or the tie row
    itself as the bias."""
    g0 = E.onehot_gemm(M, 1536, 0)
    ad, sad = dev(torch, _to_kp(g0["qx"]) if kp else g0["qx"]), dev(torch, g0["sa"])
    wd = pack_w(torch, g0["qw"], kp)
    out8, os_ = empty(torch, (3, M, 512), "int8"), empty(torch, (3, M), "float32")
    for st, kind in E.ONEHOT_QKV:
        g = E.onehot_gemm(M, 1536, st, kind)
        _rows_call(torch, A=ad, sa=sad, W=wd, sw=dev(torch, g["sw"]), bias=dev(torch, g["b"]),
                   M=M, N=1536, K=512, epi=0, out8=out8, ldo8=512, o8_ts=M * 512, os=os_,
                   os_ts=M, kp=kp)
        y = O.linear_epilogue(O.int_gemm(g["qx"], g["qw"]), g["sa"], g["sw"], g["b"])
        for t in range(3):
            q, s = O.quant_rows(y[:, 512 * t:512 * (t + 1)])
            np.testing.assert_array_equal(os_[t].cpu().numpy(), s)
            np.testing.assert_array_equal(out8[t].cpu().numpy(), q)


@pytest.mark.parametrize("M", [97, 300])
@pytest.mark.parametrize("kp", [1, 2, 3])
def test_linear_rows_ffn1(torch, kp, M):
    """epi 3: relu(y) quantized over 2048 columns, y rows = a 2048-wide tie row times
    2**(m % 5 - 2) (negative ties clamp to code 0, positive ones go through the u8
    conversion): kp = 1 and 2 in two passes (epi 2's maxima as pmax_in), kp = 3 in one pass
    (k_gemm_wsy)."""
    g0 = E.onehot_gemm(M, 2048, 0)
    ad, sad = dev(torch, _to_kp(g0["qx"])), dev(torch, g0["sa"])
    wd = pack_w(torch, g0["qw"], kp)
    nb = (M + 31) // 32
    for st, kind in E.ONEHOT_FFN1:
        g = E.onehot_gemm(M, 2048, st, kind)
        base = dict(A=ad, sa=sad, W=wd, sw=dev(torch, g["sw"]), bias=dev(torch, g["b"]), M=M,
                    N=2048, K=512, kp=kp)
        h = O.linear_epilogue(O.int_gemm(g["qx"], g["qw"]), g["sa"], g["sw"], g["b"], relu=True)
        h8 = zeros(torch, (M + (M & 1), 2048), "int8")
        sh = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
        if kp == 3:
            gx = empty(torch, ((32 * M + 2048) // 4,), "float32")
            _rows_call(torch, epi=3, pmax_out=gx, out8=h8, ldo8=2048, os=sh, **base)
            assert gx.view(torch.int32)[2 * (4 * 32 * nb) + 1].item() == 0
        else:
            pm = empty(torch, (4, M), "float32")
            _rows_call(torch, epi=2, pmax_out=pm, **base)
            np.testing.assert_array_equal(pm.cpu().numpy(), h.reshape(M, 4, 512).max(-1).T)
            _rows_call(torch, epi=3, pmax_in=pm, pmax_n=4, out8=h8, ldo8=2048, os=sh, **base)
        qh, s = O.quant_rows(h)
        np.testing.assert_array_equal(sh.cpu().numpy(), s)
        np.testing.assert_array_equal(_from_kp(h8.cpu().numpy(), M), qh)


# ----------------------------------------------------------------- encoder attention
@pytest.mark.parametrize("S", [16, 128])
def test_attention_quant(torch, S):
    """k_attn_encq's context quantizer (div_cr): one kept key per sentence, so the context is
    float(v) * s_v and its quotients sit a few ulps around +-63.5; S = 128 is the
    pipelined-heads instance."""
    B = 8
    c = E.encq_case(B, S)
    _, qc, sc = E.encq_expected(B, S)
    ctx8, sctx = empty(torch, (B, S, 512), "int8"), empty(torch, (B, S), "float32")
    call("qtx_attention_i8_quant", P(dev(torch, c["q"])), P(dev(torch, c["sq"])),
         P(dev(torch, c["k"])), P(dev(torch, c["sk"])), P(dev(torch, c["v"])),
         P(dev(torch, c["sv"])), P(dev(torch, c["km"])), B, S, P(ctx8), P(sctx), S0)
    np.testing.assert_array_equal(sctx.cpu().numpy(), sc)
    np.testing.assert_array_equal(ctx8.cpu().numpy(), qc)
