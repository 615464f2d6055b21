"""Every attention kernel's softmax on the rounding ties of the 1/127 probability grid and
their floating-point neighbours (tests/softmax_edges.py), bit-exact against the oracle.

Each kernel forms e / den with a shortcut of its own: k_attn_mfma by div_cr behind a wave-wide
range vote with the true division as the other branch, k_attn_encq and k_dec_attn by an
unguarded div_cr, k_attention and k_attn_trace by the true division.  The rows hold two live keys
whose probabilities sit on a tie k + 1/2 (every k = 0 .. 126, from both sides), the exact ties
of 2 and of 254 equal keys, and guard rows with e_B on either side of 2^-60 and of the flush
threshold; in "i8_guard" one query of every 16 (one wave of k_attn_mfma) is such a guard row,
so the true-division branch sees ties too.  That these inputs fail a kernel whose quotient,
exponential or denominator is off by an ulp, or that rounds half away from zero, is shown on the
CPU by tests/test_softmax_edges_ref.py (its counts are the sensitivity of this file); no
tolerance anywhere here.

k_attn_fault_rows is not covered: it is reachable only through the model-level fault entry
points, where the scores cannot be steered; it divides with the plain true division.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_edges as E  # noqa: E402
from test_gpu_fused import P, S0, _release, call, head_max, torch, vgroup4, vungroup4  # noqa: E402,F401
from test_gpu_fused import dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def dev(torch, a):
    """test_gpu_fused.dev on a private copy (the generator's arrays are read-only)."""
    return _dev(torch, np.array(a))


def empty(torch, shape, dtype="float32"):
    return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")


def op_args(torch, c):
    v = c["view"]
    return [P(dev(torch, v[n])) for n in ("q", "sq", "k", "sk", "v", "sv")]


def pair_codes(name):
    """The codes of a two-key case as the sweep recorded them (0 everywhere else)."""
    c = E.case(name)
    p = E.pool(c["kind"])
    B, Sq = c["jA"].shape
    Sk = c["view"]["k"].shape[1]
    b, i = np.arange(B)[:, None], np.arange(Sq)[None, :]
    s = c["src"]
    out = np.zeros((B, 8, Sq, Sk), f32)
    for h in range(8):
        out[b, h, i, c["jA"]] = np.where(s >= 0, p["code_a"][s], 127)      # (guard rows: 127, 0)
        out[b, h, i, c["jB"]] = np.where(s >= 0, p["code_b"][s], 0)
    return out


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("name", E.names("trace"))
def test_attention_trace(torch, name, dec):
    """k_attn_trace: "trace16" is one sentence with every kept row of the sweep as a query
    (Sk = 16), "trace254" the equal-key and fully masked rows.  p_codes also directly against the
    codes the sweep recorded."""
    c = E.case(name)
    v = c["view"]
    B, Sq, Sk = v["mask"].shape
    ctx = empty(torch, (B, Sq, 512))
    qk, pc = empty(torch, (B, 8, Sq, Sk)), empty(torch, (B, 8, Sq, Sk))
    call("qtx_attention_trace", *op_args(torch, c), P(dev(torch, c["mask_dev"])), c["m_bs"],
         c["m_is"], B, 8, Sq, Sk, P(ctx), P(qk), P(pc), dec, S0)
    co, qp = E.expected(name, bool(dec))
    got = pc.cpu().numpy()
    if c["pairs"]:
        np.testing.assert_array_equal(got, pair_codes(name))
    else:
        n = c["n"][0]
        for i in range(Sq):
            assert set(np.unique(got[0, :, i])) == ({0.0, 64.0} if n[i] == 2 else {0.0})
    np.testing.assert_array_equal(got, qp.astype(f32))
    acc = np.einsum("bhid,bhjd->bhij", E.O.split_heads(v["q"], 8).astype(np.int64),
                    E.O.split_heads(v["k"], 8).astype(np.int64))
    np.testing.assert_array_equal(qk.cpu().numpy(), acc.astype(f32))
    np.testing.assert_array_equal(ctx.cpu().numpy(), co)


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("name", E.names("i8"))
def test_attention_i8(torch, name, dec):
    """k_attn_mfma ("i8_128": a mask row per query, every key slot; "i8_20": partial tiles and one
    key mask per sentence; "i8_guard": a guard row in every wave) and k_attention ("i8_130",
    "i8_254", and "i8_254x": the exact ties)."""
    c = E.case(name)
    B, Sq, Sk = c["view"]["mask"].shape
    ctx = empty(torch, (B, Sq, 512))
    call("qtx_attention_i8", *op_args(torch, c), P(dev(torch, c["mask_dev"])), c["m_bs"], c["m_is"],
         B, 8, Sq, Sk, P(ctx), dec, S0)
    np.testing.assert_array_equal(ctx.cpu().numpy(), E.expected(name, bool(dec))[0])


@pytest.mark.parametrize("name", E.names("i8_quant"))
def test_attention_i8_quant(torch, name):
    """k_attn_encq: S = 128 (the pipelined instance) and S = 16; the pair moves from sentence to
    sentence.  One code step changes the row's scale, so sctx is compared first."""
    c = E.case(name)
    B, S, _ = c["view"]["mask"].shape
    ctx8, sctx = empty(torch, (B, S, 512), "int8"), empty(torch, (B, S))
    call("qtx_attention_i8_quant", *op_args(torch, c), P(dev(torch, c["mask_dev"])), B, S, P(ctx8),
         P(sctx), S0)
    qc, sc = E.expected_quant(name)
    np.testing.assert_array_equal(sctx.cpu().numpy(), sc)
    np.testing.assert_array_equal(ctx8.cpu().numpy(), qc)


@pytest.mark.parametrize("name", E.names("cross"))
def test_decode_cross_attention(torch, name):
    """k_dec_attn<false>: one query per sentence; S = 17 (one partial fragment), 64, 65 (the
    second key slot holds one key) and 128."""
    c = E.case(name)
    r = c["raw"]
    B, S = r["mask"].shape
    ctxd, pm = empty(torch, (B, 512)), empty(torch, (8, B))
    call("qtx_decode_attention", 0, P(dev(torch, r["y"])), 512, P(dev(torch, r["kc"])),
         P(dev(torch, vgroup4(r["vc"]))), P(dev(torch, r["skc"])), P(dev(torch, r["svc"])), S, S0, S,
         P(dev(torch, r["mask"])), B, P(ctxd), P(pm), S0)
    ctx = E.expected(name, True)[0][:, 0]
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx)
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx))


@pytest.mark.parametrize("name", E.names("self"))
def test_decode_self_attention(torch, name):
    """k_dec_attn<true> at the steps 1, 63, 64 and 127: no mask, the dead keys 126 below the
    maximum; the new key is key A in half of the sentences and a dead key in the others.  The
    caches and the head maxima are compared too."""
    c = E.case(name)
    r, after, step, kv_bs = c["raw"], c["after"], c["step"], c["kv_bs"]
    B = len(r["y"])
    kcd, vcd = dev(torch, r["kc"]), dev(torch, vgroup4(r["vc"]))
    skd, svd = dev(torch, r["skc"]), dev(torch, r["svc"])
    ctxd, pm = empty(torch, (B, 512)), empty(torch, (8, B))
    call("qtx_decode_attention", 1, P(dev(torch, r["y"])), 1536, P(kcd), P(vcd), P(skd), P(svd),
         kv_bs, P(dev(torch, np.array([step], np.int32))), 0, S0, B, P(ctxd), P(pm), S0)
    np.testing.assert_array_equal(kcd.cpu().numpy(), after["kc"])
    np.testing.assert_array_equal(vungroup4(vcd.cpu().numpy(), kv_bs), after["vc"])
    np.testing.assert_array_equal(skd.cpu().numpy(), after["skc"])
    np.testing.assert_array_equal(svd.cpu().numpy(), after["svc"])
    ctx = E.expected(name, True)[0][:, 0]
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx)
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx))
