"""The rounding-edge inputs (tests/rounding_edges.py) can fail a wrong quantizer — shown on the
CPU, with the oracle alone.

For every array that tests/test_gpu_rounding_edges.py feeds to a quantizing kernel, the rows
the kernel quantizes are computed here with the oracle, and three wrong quantizers are run on
them: (a) rint(fl(x * RN(1/s))) — the near-tie fallback removed, or a div_cr without its
correction step; (b) the same with the reciprocal one ulp low / high (v_rcp_f32's accuracy);
(c) the correct quotient rounded half away from zero.  Each must get at least 8 (a, b) and 16
(c) codes of every row wrong, and (a, b) at least 100 of every (mantissa, exponent) set.
These are conditions on the inputs: a construction that stops producing near-ties fails here.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounding_edges as E  # noqa: E402

f32 = np.float32
WIDTHS = (256, 512, 768, 2048)


def check_rows(x, n_bits=8, relu=False, c_min=16):
    """The per-row conditions on fp32 rows a site quantizes; returns the counts."""
    _, cnt = E.discrimination(x, n_bits, relu)
    for key in ("a", "b_lo", "b_hi"):
        assert cnt[key].min() >= 8, (key, cnt[key])
    assert cnt["c"].min() >= c_min, cnt["c"]
    return cnt


@pytest.mark.parametrize("qmax,bits", [(127.0, 8), (7.0, 4)])
@pytest.mark.parametrize("D", WIDTHS)
def test_tie_rows_exact(D, qmax, bits):
    """In rational arithmetic every tie element has x / s == k + 1/2 and the oracle gives the
    even neighbour and the scale s exactly; every k, and every neighbour of its tie, is in
    the set; the first and last four columns hold ties."""
    for mant, exp in (E.COMBOS if bits == 8 else E.COMBOS_Q7):
        x = E.tie_rows(D, mant, exp, qmax)
        s = E.scale_of(mant, exp)
        assert x.dtype == f32 and x.shape[1] == D and not x.flags.writeable
        q, so = O.quant_rows(x, bits)
        assert (so == s).all() and (np.abs(x).max(-1) == f32(qmax) * s).all()
        tie = E.tie_mask(x, s)
        assert tie[:, :4].all() and tie[:, -4:].all()
        two_q = np.array([int(Fraction(float(v)) / Fraction(float(s)) * 2) for v in x[tie]])
        k = (two_q - 1) // 2                                  # x / s == k + 1/2
        even = np.where(k % 2 == 0, k, k + 1)
        np.testing.assert_array_equal(q[tie], even)
        assert set(k) == set(range(-int(qmax), int(qmax)))
        pat, _ = E.tie_pattern(mant, exp, qmax)
        assert set(pat.reshape(-1).tolist()) <= set(x.reshape(-1).tolist())
        # every float4 chunk of every row (so every lane) holds a tie or a neighbour of one
        assert np.isin(x, pat).reshape(len(x), D // 4, 4).any(-1).all()


@pytest.mark.parametrize("qmax,bits", [(127.0, 8), (7.0, 4)])
@pytest.mark.parametrize("D", WIDTHS)
def test_tie_rows_discriminate(D, qmax, bits):
    for mant, exp in (E.COMBOS if bits == 8 else E.COMBOS_Q7):
        cnt = check_rows(E.tie_rows(D, mant, exp, qmax), bits)
        for key in ("a", "b_lo", "b_hi"):
            assert cnt[key].sum() >= 100, (mant, exp, key, cnt[key])


def check_lone(x, relu=False):
    """Rows with one near-tie each: some reciprocal model gets exactly that one code wrong."""
    _, cnt = E.discrimination(x, 8, relu)
    worst = np.maximum(np.maximum(cnt["a"], cnt["b_lo"]), cnt["b_hi"])
    assert (worst == 1).all(), worst


@pytest.mark.parametrize("D", WIDTHS)
def test_lone_rows(D):
    """A lone row: every element but one is an exact integer multiple of the scale (rational
    arithmetic), the one is positive, its row's model gets exactly its code wrong and no model
    any other; over the rows the lone element visits every (chunk group, element) slot a lane
    can hold it in, in many lanes."""
    x, cols, models = E.lone_rows(D)
    (q, s), cnt = E.discrimination(x)
    ref = q.astype(np.float64)
    for i, (row, col, model) in enumerate(zip(x, cols, models)):
        mant, exp = E.COMBOS[i % len(E.COMBOS)]
        assert s[i] == E.scale_of(mant, exp)
        fs = Fraction(float(s[i]))
        whole = np.array([(Fraction(float(v)) / fs).denominator == 1 for v in row])
        assert not whole[col] and whole.sum() == D - 1 and row[col] > 0
        ulps = dict(E.LONE_MODELS)[model]
        bad = np.flatnonzero(E.model_recip(row[None], s[i:i + 1], ulps)[0] != ref[i])
        assert bad.tolist() == [col]
        assert max(cnt[m][i] for m, _ in E.LONE_MODELS) == 1
    assert {(c // 256, c % 4) for c in cols} == {(j, e) for j in range(D // 256) for e in range(4)}
    assert len({(c // 4) % 64 for c in cols}) >= min(len(cols), 40)
    check_lone(x)


def test_rejected_mantissas():
    """Why 5, 9, 17 (and 3) are not used: model (a) gets (almost) every code right."""
    for mant, most in ((5, 0), (9, 0), (17, 0), (3, 99)):
        _, cnt = E.discrimination(E.tie_rows(2048, mant, -10), 8)
        assert cnt["a"].sum() <= most


def test_direct_rows():
    """The rows the direct-input cases use (qtx_row_quant, the skinny amode 2 / 3 prologues,
    the decode attention's q | k | v thirds)."""
    for D in WIDTHS:
        check_rows(E.all_rows(D))
        check_rows(E.all_rows(D, 7.0), 4)
    for K, M, start in [c[1:2] + c[3:] for c in E.SKINNY_DIRECT] + [E.DECODE_CROSS_Q]:
        h, lone = E.direct_rows(K, M, start)
        check_rows(h[~lone])
        check_lone(h[lone])
    check_lone(E.decode_y(3, lone=True).reshape(9, 512))
    y = E.decode_y(3)
    mants = [[int(round(np.abs(y[b, 512 * t:512 * (t + 1)]).max() / 127 * 2 ** 12)) for t in range(3)]
             for b in range(3)]
    for row in mants:       # three different mantissas per sentence (odd part of the scale)
        odd = [m // (m & -m) for m in row]
        assert len(set(odd)) == 3, row
    check_rows(y.reshape(9, 512))


def test_layernorm_gamma0_is_beta():
    """gamma = 0: LN(x) == beta bit for bit for finite non-constant x ((0 * d) / den is a signed
    zero), so the LayerNorm sites quantize exactly the beta rows."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((9, 512)) * rng.uniform(0.01, 30, (9, 1))).astype(f32)
    b = E.betas()
    assert len(b) == E.N_TIE_BETAS + 24
    for beta in b:
        ln = O.layer_norm(x, np.zeros(512, f32), beta)
        np.testing.assert_array_equal(ln, np.broadcast_to(beta, ln.shape))
        q, s = O.quant_rows(ln)
        qb, sb = O.quant_rows(beta[None])
        np.testing.assert_array_equal(q, np.broadcast_to(qb, q.shape))
        assert (s == sb[0]).all()
    check_rows(b[:E.N_TIE_BETAS])
    check_lone(b[E.N_TIE_BETAS:])


@pytest.mark.parametrize("M", [97, 300])
def test_onehot_gemm_rows(M):
    """The GEMM-epilogue construction: every product exact, so row m of y is the tie row times
    2**(m % 5 - 2) (kind "bias": the bias row itself); Q/K/V tiles (512 wide) and the ReLU'd
    FFN1 hidden (2048 wide)."""
    for N, starts, relu in ((1536, E.ONEHOT_QKV, False), (2048, E.ONEHOT_FFN1, True)):
        for st, kind in starts:
            g = E.onehot_gemm(M, N, st, kind)
            lone = kind == "lone"
            y = O.linear_epilogue(O.int_gemm(g["qx"], g["qw"]), g["sa"], g["sw"], g["b"])
            exact = g["sa"].astype(np.float64)[:, None] * g["sw"].astype(np.float64)[None, :]
            np.testing.assert_array_equal(y.astype(np.float64), exact + g["b"].astype(np.float64))
            assert (exact == 0).all() if kind == "bias" else not g["b"].any()
            for t in range(N // 512 if not relu else 1):
                tile = y if relu else y[:, 512 * t:512 * (t + 1)]
                (check_lone if lone else check_rows)(tile, relu=relu)
                _, s = O.quant_rows(np.maximum(tile, 0) if relu else tile)
                assert len(set(s.tolist())) == (1 if kind == "bias" else 5)   # scales per call


def test_ffn_hidden_rows():
    """The fused FFN's hidden quantizer with A = 0: h = relu(b1)."""
    for F in (256, 2048):
        for st in E.FFN_HIDDEN_STARTS:
            b1 = E.ffn_hidden_bias(F, st)
            check_rows(b1[None], relu=True)
            assert (b1 < 0).sum() >= 8           # some ties still go through the clamp at 0


@pytest.mark.parametrize("S", [16, 128])
def test_encq_context_rows(S):
    """One kept key per sentence: the context of every query is float(v) * s_v of that key,
    whose quotients sit a few ulps around +-63.5.  No exact ties, so only the reciprocal
    models apply; (a) is k_attn_encq's div_cr without its correction."""
    B = 8
    c = E.encq_case(B, S)
    ctx, qc, sc = E.encq_expected(B, S)
    assert (c["km"].sum(-1) == 1).all() and len(set(c["keep"].tolist())) == B
    for b in range(B):
        row = c["v"][b, c["keep"][b]].astype(f32) * c["sv"][b, c["keep"][b]]
        np.testing.assert_array_equal(ctx[b], np.broadcast_to(row, (S, 512)))
        assert np.abs(c["v"][b, c["keep"][b]]).max() == 2
    distinct = ctx[:, 0]
    quo = np.abs(distinct[np.abs(distinct) > 0].astype(np.float64)
                 / np.repeat(sc[:, 0], (np.abs(distinct) > 0).sum(-1)))
    assert ((np.abs(quo - 63.5) < 1e-4) | (np.abs(quo - 127) < 1e-4)).all()
    _, cnt = E.discrimination(distinct)
    assert cnt["a"].min() >= 8, cnt["a"]
