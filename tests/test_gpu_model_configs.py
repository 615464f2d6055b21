"""Every model config qtx_model_create accepts, and the library's path switches, against the
oracle — bit for bit.

The host code picks whole kernel chains from the config (csrc/qtx_api.hip): the row-GEMM
chain needs d_ff % 512 == 0, the weight-stationary kernels a K = 512 GEMM over many rows, the
one-pass FFN1 d_ff == 2048, the fused decode step d_ff in {512, 2048} and a vocabulary of at
most 8192; everything else runs the generic k_gemm chain and the unfused step.  The rule
these tests enforce: no config is accepted at creation and then fails in a later call.

Models are small (tests/model_cfgs.py: 2 layers, 64 / 97 words), so each case takes a
fraction of a second; B, S = 3, 50 gives 150 rows — two 128-row tiles, the second ragged.
Expected values come from oracle/qtx_oracle.py alone; the oracle's results are memoized and
shared between the path variants of one config.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O
from qtx import fault as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_cfgs as MC  # noqa: E402
from test_gpu_scored import gpu_scored, oracle_scored_decode  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
_MEMO = {}
ENC_B, ENC_S, DEC_T = 3, 50, 6          # 150 encoder rows: a full and a ragged row tile
GR_B, GR_S, GR_L = 3, 9, 9              # the greedy decode (model_cfgs.py: the seeds' guard)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def models(torch):
    """get(d_ff, weight_bits = 8, tgt_vocab = 97) -> (QtxModel, OracleModel), built once."""
    from qtx.model import QtxModel
    cache = {}

    def get(d_ff, weight_bits=8, tgt_vocab=97):
        key = (d_ff, weight_bits, tgt_vocab)
        if key not in cache:
            cfg, sd, om = MC.small_state(*key)
            cache[key] = (QtxModel(sd, cfg), om)
        return cache[key]
    yield get
    cache.clear()


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def T_(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u8(torch, m):
    return T_(torch, np.asarray(m).reshape(m.shape[0], m.shape[-1]).astype(np.uint8))


# ---- inputs and oracle results, one set per model key -------------------------------------
def enc_case(key, om, vocab=64):
    """(x [3,50,512], mask, oracle memory): sentences 0 and 1 padded, sentence 2 (rows
    100 .. 149, so every row of the second row tile) full length."""
    def make():
        src, m = MC.small_src(ENC_B, ENC_S, 17, vocab, full=(2,))
        assert (src[:2] == 2).any(axis=1).all() and not (src[2] == 2).any()
        x = om.embed(src, om.src_lut)
        return x, m, om.encode(x, m)
    return memo(("enc", key), make)


def dec_case(key, om, vocab=97):
    """(y [3,6,512], tril mask, oracle decoder output) on the oracle's memory of enc_case."""
    def make():
        x, m, memory = enc_case(key, om)
        ys = np.random.default_rng(23).integers(4, vocab, (ENC_B, DEC_T))
        y = om.embed(ys, om.tgt_lut)
        tm = np.tril(np.ones((1, DEC_T, DEC_T), np.uint8))
        return y, tm, om.decode(y, memory, m, tm)
    return memo(("dec", key), make)


def greedy_case(key, om, B=GR_B, S=GR_S, L=GR_L, vocab=64):
    """(src, mask, the oracle's scored decode: ys, top_ids, top_logp).  Guard: some sentence
    holds at least three distinct tokens after the start symbol."""
    def make():
        src, m = MC.small_src(B, S, 5, vocab, full=(0,))
        ys, ti, tv = oracle_scored_decode(om, src, m, L)
        np.testing.assert_array_equal(ys, om.greedy_decode(src, m, L))
        assert MC.distinct_tokens(ys) >= 3, ys
        return src, m, ys, ti, tv
    return memo(("greedy", key, B, S, L), make)


def gpu_encode(torch, gm, x, m, fault=None):
    return gm.encode(T_(torch, x), u8(torch, m), fault=fault).cpu().numpy()


def gpu_decode(torch, gm, y, memory, m, tm, fault=None):
    return gm.decode(T_(torch, y), T_(torch, memory), u8(torch, m), T_(torch, tm[0]),
                     fault=fault).cpu().numpy()


def gpu_greedy(gm, src, m, L):
    from qtx.decode import greedy_decode
    return greedy_decode(gm, src, m, L, 0)


def check_model(torch, gm, om, key):
    """encode, decode and greedy of one model == the oracle (the current switches)."""
    x, m, memory = enc_case(key, om)
    np.testing.assert_array_equal(gpu_encode(torch, gm, x, m), memory)
    y, tm, ref = dec_case(key, om)
    np.testing.assert_array_equal(gpu_decode(torch, gm, y, memory, m, tm), ref)
    src, sm, ys, _, _ = greedy_case(key, om)
    np.testing.assert_array_equal(gpu_greedy(gm, src, sm, GR_L), ys)


# =====================================================================================
# 0. the row quantizer / LayerNorm at every width a model's d_ff can give it
# =====================================================================================
@pytest.mark.parametrize("D", [256 * k for k in range(1, 9)])
def test_row_quant_every_width(torch, D):
    """qtx_model_create quantizes w_2 [512, d_ff] and the generic chain the FFN hidden
    [M, d_ff] with rows of d_ff floats: every multiple of 256 up to 2048 (9 rows: three
    workgroups, the last ragged; a zero row, a row of exact ties, the int4 quantizer)."""
    from qtx import _lib
    rng = np.random.default_rng(D)
    R = 9
    x = (rng.standard_normal((R, D)) * rng.uniform(1e-3, 10, (R, 1))).astype(f32)
    x[0] = 0
    x[1] = 0
    x[1, -4:] = [127.0, 0.5, 1.5, -2.5]
    xd = T_(torch, x)
    P = lambda t: C.c_void_p(t.data_ptr())
    for qmax, bits in ((127.0, 8), (7.0, 4)):
        q = torch.full((R + 1, D), 99, dtype=torch.int8, device="cuda")
        s = torch.full((R + 1,), -1.0, dtype=torch.float32, device="cuda")
        _lib.call("qtx_row_quant", P(xd), R, D, qmax, P(q), P(s), C.c_void_p(0))
        qo, so = O.quant_rows(x, bits)
        np.testing.assert_array_equal(q[:R].cpu().numpy(), qo)
        np.testing.assert_array_equal(s[:R].cpu().numpy(), so)
        assert (q[R] == 99).all() and s[R] == -1.0          # nothing past the last row
    if D % 512:       # the widths this change opens: the LayerNorm form too
        a = rng.uniform(0.5, 1.5, D).astype(f32)
        b = rng.uniform(-0.1, 0.1, D).astype(f32)
        ad, bd = T_(torch, a), T_(torch, b)      # (named: they must outlive the call)
        y = torch.empty((R, D), dtype=torch.float32, device="cuda")
        _lib.call("qtx_layernorm_quant", P(xd), P(ad), P(bd), R, D, P(y), None, None,
                  C.c_void_p(0))
        np.testing.assert_array_equal(y.cpu().numpy(), O.layer_norm(x, a, b))
    xb = torch.zeros((R, 128), device="cuda")
    with pytest.raises(_lib.QtxError) as e:                  # not a multiple of 256
        _lib.call("qtx_row_quant", P(xb), R, 128, 127.0, P(q), P(s), C.c_void_p(0))
    assert e.value.code == 4


# =====================================================================================
# 1. the config matrix
# =====================================================================================
@pytest.mark.parametrize("d_ff", MC.D_FFS)
def test_config_encode(torch, models, d_ff):
    gm, om = models(d_ff)
    x, m, memory = enc_case((d_ff, 8, 97), om)
    np.testing.assert_array_equal(gpu_encode(torch, gm, x, m), memory)


@pytest.mark.parametrize("d_ff", MC.D_FFS)
def test_config_decode(torch, models, d_ff):
    """Teacher-forced decoder run (T = 6, causal mask) on the oracle's memory."""
    gm, om = models(d_ff)
    key = (d_ff, 8, 97)
    x, m, memory = enc_case(key, om)
    y, tm, ref = dec_case(key, om)
    np.testing.assert_array_equal(gpu_decode(torch, gm, y, memory, m, tm), ref)


@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_UNFUSED": 1}],
                         ids=["default", "nograph", "unfused"])
@pytest.mark.parametrize("d_ff", MC.D_FFS)
def test_config_greedy(torch, models, knob_env, d_ff, env):
    gm, om = models(d_ff)
    src, m, ys, _, _ = greedy_case((d_ff, 8, 97), om)
    for k, v in env.items():
        knob_env(k, v)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, GR_L), ys)


@pytest.mark.parametrize("d_ff", MC.D_FFS)
def test_config_scored_greedy(torch, models, d_ff):
    gm, om = models(d_ff)
    src, m, ys, ti, tv = greedy_case((d_ff, 8, 97), om)
    gy, gi, gv = gpu_scored(gm, src, m, GR_L)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)


@pytest.mark.parametrize("d_ff", [512, 1024])
def test_config_greedy_large_batch(torch, models, d_ff):
    """B = 100: from 96 rows the fused step (d_ff 512) quantizes the FFN hidden with its own
    kernel and runs the int8 FFN2 and the wide skinny kernels; d_ff 1024 decodes unfused."""
    gm, om = models(d_ff)
    src, m, ys, ti, tv = greedy_case((d_ff, 8, 97), om, B=100, S=9, L=5)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, 5), ys)
    gy, gi, gv = gpu_scored(gm, src, m, 5)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)


@pytest.mark.parametrize("d_ff", [256, 512, 1024])
def test_config_int4(torch, models, d_ff):
    """weight_bits = 4 against OracleModel(n_bits = 4).  d_ff 256: the int4 staging buffer
    of qtx_model_create must hold a 512 x 512 linear, not only d_ff x 512."""
    gm, om = models(d_ff, 4)
    key = (d_ff, 4, 97)
    check_model(torch, gm, om, key)
    src, m, ys, ti, tv = greedy_case(key, om)
    gy, gi, gv = gpu_scored(gm, src, m, GR_L)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)
    # a different model from the 8-bit one of the same seed
    assert not np.array_equal(enc_case(key, om)[2],
                              enc_case((d_ff, 8, 97), MC.small_state(d_ff)[2])[2])


@pytest.mark.diag
@pytest.mark.parametrize("d_ff", [256, 512, 1024])
def test_config_int4_packed_step(torch, models, knob_env, d_ff):
    """The diagnostic build's decode step on the packed int4 kernels (QTX_INT4_PACKED; the
    fused step of d_ff 512) gives the oracle's ids as well."""
    gm, om = models(d_ff, 4)
    src, m, ys, _, _ = greedy_case((d_ff, 4, 97), om)
    knob_env("QTX_INT4_PACKED", 1)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, GR_L), ys)


def test_config_large_vocab(torch, models):
    """tgt_vocab = 8200 is above the fused tail's cap (8192): plain and scored greedy take
    the unfused step and equal the oracle; the per-op tail keeps its documented cap."""
    from qtx import _lib
    key = (512, 8, 8200)
    gm, om = models(*key)
    src, m, ys, ti, tv = greedy_case(key, om)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, GR_L), ys)
    gy, gi, gv = gpu_scored(gm, src, m, GR_L)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)
    P = lambda t: C.c_void_p(t.data_ptr())
    logits = torch.zeros((1, 8200), device="cuda")
    ids = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    step = torch.zeros(4, dtype=torch.int32, device="cuda")
    xn = torch.zeros((1, 512), device="cuda")
    with pytest.raises(_lib.QtxError) as e:
        _lib.call("qtx_decode_argmax_embed", gm.handle, P(logits), 1, P(ids), 4, P(step), P(xn),
                  C.c_void_p(0))
    assert e.value.code == 4


# ---- faults on the FFN at the coordinates that depend on d_ff --------------------------
def ffn_faults(d_ff, module, rows):
    """FFN1 / FFN2 faults at the last column, row or window of d_ff; rows: the module's token
    rows (encoder: the fault row, 148, is an unmasked token of the second, ragged row tile)."""
    r = rows - 2
    return [F.Fault("INPUT16", module, 1, "FFN1", row=r, col=300, bit=7, win_start=d_ff - 16,
                    win_len=16),
            F.Fault("WEIGHT", module, 0, "FFN1", row=d_ff - 1, col=511, bit=6),
            F.Fault("RANDOM", module, 1, "FFN1", row=r, col=d_ff - 1, value=37.5),
            F.Fault("INPUT", module, 0, "FFN2", row=r, col=d_ff - 1, bit=7),
            F.Fault("WEIGHT", module, 1, "FFN2", row=511, col=d_ff - 1, bit=6)]


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("module", [0, 1], ids=["enc", "dec"])
@pytest.mark.parametrize("d_ff", [256, 1024])
def test_config_ffn_fault(torch, models, d_ff, module, i):
    """d_ff 256 runs the generic chain (k_gemm carries the fault), d_ff 1024 the row GEMM."""
    gm, om = models(d_ff)
    key = (d_ff, 8, 97)
    x, m, memory = enc_case(key, om)
    if module == 0:
        f = ffn_faults(d_ff, 0, ENC_B * ENC_S)[i]
        ref = memo(("ffault", key, 0, i), lambda: om.encode(x, m, fault=f.as_dict()))
        assert not np.array_equal(ref, memory)            # bit 6 / 7: not a golden run
        np.testing.assert_array_equal(gpu_encode(torch, gm, x, m, fault=f), ref)
    else:
        y, tm, gold = dec_case(key, om)
        f = ffn_faults(d_ff, 1, ENC_B * DEC_T)[i]
        ref = memo(("ffault", key, 1, i), lambda: om.decode(y, memory, m, tm, fault=f.as_dict()))
        assert not np.array_equal(ref, gold)
        np.testing.assert_array_equal(gpu_decode(torch, gm, y, memory, m, tm, fault=f), ref)


@pytest.mark.parametrize("d_ff", [256, 1024])
def test_config_ffn_fault_bounds(torch, models, d_ff):
    """row / col = d_ff is one past the end: QTX_E_INVALID, on every chain."""
    from qtx._lib import QtxError
    gm, om = models(d_ff)
    x, m, _ = enc_case((d_ff, 8, 97), om)
    bad = [F.Fault("WEIGHT", 0, 0, "FFN1", row=d_ff, col=0, bit=1),
           F.Fault("RANDOM", 0, 0, "FFN1", row=0, col=d_ff, value=1.0),
           F.Fault("INPUT", 0, 0, "FFN2", row=0, col=d_ff, bit=1),
           F.Fault("WEIGHT", 0, 0, "FFN2", row=0, col=d_ff, bit=1),
           F.Fault("INPUT16", 0, 0, "FFN1", row=0, col=0, bit=1, win_start=d_ff - 15, win_len=16)]
    for f in bad:
        with pytest.raises(QtxError) as e:
            gpu_encode(torch, gm, x, m, fault=f)
        assert e.value.code == 1, f


# ---- every other fault target on the generic chain (d_ff 256) ---------------------------
# The chain's GEMM (k_gemm) and attention carry the faults the row-GEMM chain carries: the
# Q|K|V and CK|CV offsets, the residual epilogues, the attention MatMuls.  Encoder rows: 150
# (S = 50 keys); decoder: T = 6 queries on the 50 memory tokens per sentence.
_E, _S, _T = ENC_B * ENC_S, ENC_S, DEC_T
GENERIC_FAULTS = [
    F.Fault("WEIGHT", 0, 0, "Q", row=511, col=0, bit=7),
    F.Fault("INPUT16", 0, 1, "K", row=_E - 1, col=511, bit=7, win_start=496, win_len=16),
    F.Fault("WEIGHT16", 0, 0, "V", row=0, col=77, bit=7, win_start=120, win_len=16),
    F.Fault("RANDOM", 0, 1, "O", row=128, col=511, value=-30.0),
    F.Fault("INPUT", 0, 0, "O", row=127, col=0, bit=6),
    F.Fault("WEIGHT", 0, 1, "QK", row=2 * _S + 49, col=7 * 64 + 63, bit=7),
    F.Fault("INPUT16", 0, 0, "PV", row=2 * _S + 3, col=4 * _S + 3, bit=7, win_start=48, win_len=16),
    F.Fault("RANDOM", 0, 1, "QK", row=2 * _S + 9, col=1 * _S + 40, value=500.0),
    F.Fault("INPUT", 1, 0, "Q", row=3 * _T - 1, col=511, bit=7),
    F.Fault("WEIGHT", 1, 1, "K", row=0, col=511, bit=7),
    F.Fault("RANDOM", 1, 0, "O", row=_T, col=0, value=25.0),
    F.Fault("WEIGHT", 1, 1, "CQ", row=511, col=3, bit=7),
    F.Fault("WEIGHT", 1, 0, "CK", row=511, col=9, bit=7),
    F.Fault("INPUT", 1, 1, "CK", row=_E - 1, col=0, bit=7),
    F.Fault("WEIGHT16", 1, 1, "CV", row=0, col=100, bit=7, win_start=130, win_len=16),
    F.Fault("INPUT16", 1, 0, "CO", row=2 * _T + 5, col=200, bit=7, win_start=0, win_len=16),
    F.Fault("WEIGHT", 1, 1, "CQK", row=2 * _S + 49, col=64, bit=7),
    F.Fault("INPUT", 1, 0, "CPV", row=2 * _T + 5, col=6 * _S + 49, bit=7),
    F.Fault("WEIGHT16", 1, 1, "PV", row=2 * _T + 1, col=5 * 64, bit=7, win_start=_T - 2, win_len=2),
]


def _fault_id(f):
    return f"{'enc' if f.module == 0 else 'dec'}-{f.linear}-{f.kind}"


@pytest.mark.parametrize("f", GENERIC_FAULTS, ids=_fault_id)
def test_generic_chain_fault(torch, models, f):
    gm, om = models(256)
    key = (256, 8, 97)
    x, m, memory = enc_case(key, om)
    if f.module == 0:
        ref = om.encode(x, m, fault=f.as_dict())
        assert not np.array_equal(ref, memory)
        np.testing.assert_array_equal(gpu_encode(torch, gm, x, m, fault=f), ref)
    else:
        y, tm, gold = dec_case(key, om)
        ref = om.decode(y, memory, m, tm, fault=f.as_dict())
        assert not np.array_equal(ref, gold)
        np.testing.assert_array_equal(gpu_decode(torch, gm, y, memory, m, tm, fault=f), ref)


@pytest.mark.parametrize("f", [
    F.Fault("INPUT", 0, 1, "FFN1", row=299, col=511, bit=7),
    F.Fault("WEIGHT16", 0, 0, "FFN2", row=511, col=255, bit=7, win_start=250, win_len=16),
    F.Fault("RANDOM", 0, 1, "K", row=256, col=0, value=40.0)], ids=_fault_id)
def test_generic_chain_fault_large_tiles(torch, models, f):
    """From 256 rows k_gemm runs 128 x 128 tiles (a faulty GEMM never takes k_gemm256):
    300 rows, faults in the third, ragged row tile and across the second tile's edge."""
    gm, om = models(256)

    def make():
        src, m = MC.small_src(6, 50, 31, full=(5,))
        x = om.embed(src, om.src_lut)
        return x, m, om.encode(x, m)
    x, m, memory = memo("enc300", make)
    ref = om.encode(x, m, fault=f.as_dict())
    assert not np.array_equal(ref, memory)
    np.testing.assert_array_equal(gpu_encode(torch, gm, x, m, fault=f), ref)
    np.testing.assert_array_equal(gpu_encode(torch, gm, x, m), memory)


# =====================================================================================
# 2. path switches on the default model (6 layers, d_ff 2048) and on d_ff 1024
# =====================================================================================
SWITCHES = [{"QTX_NO_ROWGEMM": 1}, {"QTX_NO_KP": 1}, {"QTX_WS_MIN_M": 1, "QTX_WS_RES_MIN_M": 1}]
SWITCH_IDS = ["no_rowgemm", "no_kp", "ws_small_m"]


def default_case(oracle_model):
    def make():
        rng = np.random.default_rng(29)
        src = np.full((ENC_B, ENC_S), 2, np.int64)
        for b, n in enumerate((ENC_S, 31, 7)):
            src[b, 0], src[b, n - 1] = 0, 1
            src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        m = (src != 2)[:, None, :]
        x = oracle_model.embed(src, oracle_model.src_lut)
        memory = oracle_model.encode(x, m)
        y = oracle_model.embed(rng.integers(4, 4444, (ENC_B, DEC_T)), oracle_model.tgt_lut)
        tm = np.tril(np.ones((1, DEC_T, DEC_T), np.uint8))
        out = oracle_model.decode(y, memory, m, tm)
        gs = np.full((2, 12), 2, np.int64)
        for b, n in enumerate((12, 8)):
            gs[b, 0], gs[b, n - 1] = 0, 1
            gs[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        gsm = (gs != 2)[:, None, :]
        return x, m, memory, y, tm, out, gs, gsm, oracle_model.greedy_decode(gs, gsm, GR_L)
    return memo("default", make)


@pytest.mark.parametrize("env", SWITCHES, ids=SWITCH_IDS)
def test_switch_paths_default_model(torch, gpu_model, oracle_model, knob_env, env):
    """QTX_NO_ROWGEMM: the generic chain (self_attn_block / cross_attn_block / ffn_block);
    QTX_NO_KP: the row GEMMs on row-major operands; QTX_WS_MIN_M = QTX_WS_RES_MIN_M = 1: the
    weight-stationary Q/K/V, O projection and one-pass FFN1 at a small ragged M."""
    x, m, memory, y, tm, out, gs, gsm, ys = default_case(oracle_model)
    for k, v in env.items():
        knob_env(k, v)
    np.testing.assert_array_equal(gpu_encode(torch, gpu_model, x, m), memory)
    np.testing.assert_array_equal(gpu_decode(torch, gpu_model, y, memory, m, tm), out)
    np.testing.assert_array_equal(gpu_greedy(gpu_model, gs, gsm, GR_L), ys)


@pytest.mark.parametrize("env", SWITCHES, ids=SWITCH_IDS)
def test_switch_paths_dff1024(torch, models, knob_env, env):
    """d_ff 1024 under the same switches; with the weight-stationary pair, FFN1 runs its two
    passes on the weight-stationary kernel with N = 1024 (two column slices, pmax_n = 2)."""
    gm, om = models(1024)
    for k, v in env.items():
        knob_env(k, v)
    check_model(torch, gm, om, (1024, 8, 97))
