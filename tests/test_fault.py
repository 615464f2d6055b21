"""Fault injection: the reference's fault models on the qtx path.

CPU tests: MatMul-name mapping, fault drawing, the oracle's fault semantics (a flipped
int8 operand propagated through the MatMul == the MatMul recomputed on the flipped
operand, windows, RANDOM outputs).  GPU tests: encoder / decoder forward and greedy decode
with a fault == the oracle with the same fault, bit for bit."""
import numpy as np
import pytest

from oracle import qtx_oracle as O
from qtx import fault as F

f32 = np.float32


def test_matmul_names():
    assert F.matmul_target("MatMul_6", "Encoder") == (0, 0, "FFN1")      # matmul_6.json
    assert F.matmul_target("MatMul_47", "Encoder") == (0, 5, "FFN2")
    assert F.matmul_target("MatMul_13", "Encoder") == (0, 1, "O")
    assert F.matmul_target("MatMul_0", "Decoder") == (1, 0, "CK")
    assert F.matmul_target("MatMul_11", "Decoder") == (1, 5, "CV")
    assert F.matmul_target("MatMul_12", "Decoder") == (1, 0, "Q")
    assert F.matmul_target("MatMul_22", "Decoder") == (1, 0, "FFN1")     # matmul_22.json
    assert F.matmul_target("MatMul_23", "Decoder") == (1, 0, "FFN2")     # matmul_23.json
    assert F.matmul_target("MatMul_82", "Decoder") == (1, 5, "FFN1")
    assert F.matmul_target("MatMul_3", "Encoder") == (0, 0, "QK")       # matmul_3.json
    assert F.matmul_target("MatMul_12", "Encoder") == (0, 1, "PV")
    for bad in ("Add_3", "MatMul_48"):
        with pytest.raises(ValueError):
            F.matmul_target(bad, "Encoder")
    assert F.matmul_target("MatMul_15", "Decoder") == (1, 0, "QK")       # matmul_15.json
    assert F.matmul_target("MatMul_16", "Decoder") == (1, 0, "PV")
    assert F.matmul_target("MatMul_19", "Decoder") == (1, 0, "CQK")      # matmul_19.json
    assert F.matmul_target("MatMul_20", "Decoder") == (1, 0, "CPV")


def test_reference_target_files_map():
    """Every target of the reference's campaign files (QK^T, PV, FFN1, FFN2 per layer)
    maps to the matching (module, layer, target)."""
    import json
    import os
    # the campaign files' contents, stored as data by tests/golden/make_matmul_targets.py
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "matmul_targets.json")) as fh:
        targets = json.load(fh)
    n = {"Encoder": 0, "Decoder": 0}
    for j in targets:
        mod, kind = j["module"].split("/")[:2]        # FirstFC / SecondFC / First|SecondMatMul
        _, _, lin = F.matmul_target(j["target_layer"], j["module"])
        want = {"FirstFC": ("FFN1",), "SecondFC": ("FFN2",), "FirstMatMul": ("QK", "CQK"),
                "SecondMatMul": ("PV", "CPV")}[kind]
        assert lin in want, (j, lin)
        n[mod] += 1
    assert n == {"Encoder": 24, "Decoder": 36}


def test_random_fault_draws():
    rng = np.random.default_rng(0)
    for kind in ("INPUT", "WEIGHT", "INPUT16", "WEIGHT16", "RANDOM"):
        f = F.random_fault(rng, kind, 0, 2, "FFN1", rows=40, bit=3)
        N, K = F.linear_shape("FFN1")
        if kind.startswith("INPUT"):
            assert 0 <= f.row < 40 and 0 <= f.col < K
        elif kind.startswith("WEIGHT"):
            assert 0 <= f.row < N and 0 <= f.col < K
        if kind == "INPUT16":
            assert f.win_start % 16 == 0 and f.win_len == 16
        if kind == "WEIGHT16":
            assert f.win_start % 16 == 0 and 1 <= f.win_len <= 15
    g = np.ones((40, 2048), f32)
    f = F.random_fault(rng, "RANDOM_BITFLIP", 0, 0, "FFN1", 40, golden_output=g)
    assert f.value != 1.0
    f = F.from_inject_parameters({"inject_type": "WEIGHT", "faulty_operation_name": "MatMul_14",
                                  "targetted_module": "Encoder", "faulty_bit_position": 7}, 16, rng)
    assert (f.module, f.layer, f.linear, f.bit) == (0, 1, "FFN1", 7)


def _lin(rng, N=64, K=128):
    return O.QLinear(rng.standard_normal((N, K)).astype(f32) * 0.1,
                     rng.standard_normal(N).astype(f32) * 0.1)


def test_oracle_input_fault_is_flipped_operand():
    rng = np.random.default_rng(1)
    lin = _lin(rng)
    x = rng.standard_normal((10, 128)).astype(f32)
    qx, sx = O.quant_rows(x)
    flipped = qx.copy()
    flipped[3, 17] = np.int8(np.uint8(flipped[3, 17].view(np.uint8) ^ 64).view(np.int8))
    want = O.linear_epilogue(O.int_gemm(flipped, lin.q), sx, lin.s, lin.b)
    got = lin(x, fault=dict(kind="INPUT", row=3, col=17, bit=6, lo=0, hi=64, value=0))
    np.testing.assert_array_equal(got, want)
    golden = lin(x)
    w16 = lin(x, fault=dict(kind="INPUT16", row=3, col=17, bit=6, lo=16, hi=32, value=0))
    np.testing.assert_array_equal(w16[:, 16:32], want[:, 16:32])
    np.testing.assert_array_equal(w16[:, :16], golden[:, :16])
    np.testing.assert_array_equal(w16[:, 32:], golden[:, 32:])


def test_oracle_weight_and_output_faults():
    rng = np.random.default_rng(2)
    lin = _lin(rng)
    x = rng.standard_normal((12, 128)).astype(f32)
    golden = lin(x)
    wf = lin(x, fault=dict(kind="WEIGHT", row=5, col=9, bit=7, lo=0, hi=12, value=0))
    diff = np.argwhere(wf != golden)
    assert set(diff[:, 1]) <= {5}
    w16 = lin(x, fault=dict(kind="WEIGHT16", row=5, col=9, bit=7, lo=4, hi=8, value=0))
    np.testing.assert_array_equal(w16[4:8], wf[4:8])
    np.testing.assert_array_equal(w16[:4], golden[:4])
    of = lin(x, relu=True, fault=dict(kind="OUTPUT", row=2, col=3, bit=0, lo=0, hi=0, value=-7.0))
    g = lin(x, relu=True)
    assert of[2, 3] == 0.0 and np.sum(of != g) <= 1


# ------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _enc_inputs(oracle_model, B, S, seed):
    rng = np.random.default_rng(seed)
    src = np.full((B, S), 2, np.int64)
    for b, n in enumerate(rng.integers(4, S + 1, B)):
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, 5337, max(n - 2, 0))
    m = (src != 2)[:, None, :]
    return src, m, oracle_model.embed(src, oracle_model.src_lut)


ENC_CASES = [("INPUT", "FFN1", 3), ("INPUT16", "FFN2", 5), ("WEIGHT", "Q", 7), ("WEIGHT16", "FFN1", 6),
             ("RANDOM", "O", 0), ("INPUT", "V", 2), ("WEIGHT", "K", 4), ("RANDOM", "FFN1", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,linear,bit", ENC_CASES)
def test_encoder_fault_matches_oracle(torch_gpu, gpu_model, oracle_model, kind, linear, bit):
    torch = torch_gpu
    B, S = 3, 24
    src, m, x = _enc_inputs(oracle_model, B, S, 11)
    rng = np.random.default_rng(hash((kind, linear)) % 2**32)
    f = F.random_fault(rng, kind, 0, int(rng.integers(6)), linear, B * S, bit=bit)
    if kind == "RANDOM":
        f.value = float(rng.standard_normal() * 50)
    xd = torch.from_numpy(x).cuda()
    md = torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda()
    out = gpu_model.encode(xd, md, fault=f).cpu().numpy()
    ref = oracle_model.encode(x, m, fault=f.as_dict())
    np.testing.assert_array_equal(out, ref)
    if kind != "WEIGHT16":          # a golden run differs (WEIGHT16 may hit pad rows only)
        assert not np.array_equal(out, gpu_model.encode(xd, md).cpu().numpy()) or bit < 6


@pytest.mark.gpu
@pytest.mark.parametrize("kind,linear", [("WEIGHT", "CK"), ("INPUT", "CV"), ("INPUT16", "FFN1"),
                                         ("WEIGHT16", "Q"), ("RANDOM", "CO"), ("INPUT", "CQ")])
def test_decoder_fault_matches_oracle(torch_gpu, gpu_model, oracle_model, kind, linear):
    torch = torch_gpu
    B, S, T = 2, 20, 6
    src, m, x = _enc_inputs(oracle_model, B, S, 12)
    rng = np.random.default_rng(7)
    memory = oracle_model.encode(x, m)
    ys = rng.integers(4, 4444, (B, T))
    y = oracle_model.embed(ys, oracle_model.tgt_lut)
    tm = np.tril(np.ones((1, T, T), np.uint8))
    rows = B * S if linear in ("CK", "CV") else B * T
    f = F.random_fault(rng, kind, 1, int(rng.integers(6)), linear, rows, bit=6)
    if kind == "RANDOM":
        f.value = -123.5
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = gpu_model.decode(T_(y), T_(memory), T_(m.reshape(B, S).astype(np.uint8)),
                           T_(tm[0]), fault=f).cpu().numpy()
    ref = oracle_model.decode(y, memory, m, tm, fault=f.as_dict())
    np.testing.assert_array_equal(out, ref)


@pytest.mark.gpu
def test_greedy_decode_with_encoder_fault(torch_gpu, gpu_model, oracle_model):
    torch = torch_gpu
    B, S = 2, 16
    src, m, _ = _enc_inputs(oracle_model, B, S, 13)
    f = F.Fault("WEIGHT", 0, 2, "FFN2", row=17, col=100, bit=7)
    ids = gpu_model.greedy(torch.from_numpy(src).cuda(),
                           torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda(),
                           max_len=12, fault=f).cpu().numpy()
    ref = oracle_model.greedy_decode(src, m, max_len=12, fault=f.as_dict())
    np.testing.assert_array_equal(ids, ref)


@pytest.mark.gpu
def test_fault_bad_index_rejected(torch_gpu, gpu_model):
    torch = torch_gpu
    from qtx._lib import QtxError
    x = torch.zeros((1, 8, 512), device="cuda")
    md = torch.ones((1, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(QtxError):
        gpu_model.encode(x, md, fault=F.Fault("INPUT", 0, 0, "FFN1", row=8, col=0))
    with pytest.raises(QtxError):
        gpu_model.encode(x, md, fault=F.Fault("WEIGHT", 0, 0, "CK", row=0, col=0))


@pytest.mark.gpu
def test_run_module_inject_parameters(torch_gpu, gpu_model, oracle_model, golden_model):
    """run_module with the reference's inject_parameters dict (FFN target of a campaign
    file, input/encoder/matmul_6.json) == the oracle with the drawn fault."""
    from qtx.session import run_module
    feeds = {"global_in": golden_model["enc_in"], "global_in_1": golden_model["src_mask"]}
    p = {"inject_type": "INPUT", "faulty_operation_name": "MatMul_6",
         "targetted_module": "Encoder", "faulty_bit_position": 7}
    outs, wd = run_module("Encoder", feeds, None, {}, None, inject_parameters=p,
                          model=gpu_model, rng=np.random.default_rng(3))
    f = wd["qtx_fault"]
    assert (f.module, f.layer, f.linear, f.bit) == (0, 0, "FFN1", 7)
    ref = oracle_model.encode(golden_model["enc_in"], golden_model["src_mask"], fault=f.as_dict())
    np.testing.assert_array_equal(outs["global_out"], ref)


@pytest.mark.gpu
def test_run_module_fault_for_other_module_is_golden(torch_gpu, gpu_model, oracle_model,
                                                     golden_model):
    """An INPUT fault aimed at the decoder leaves an encoder run golden, as the reference's
    `module in inject_parameters["targetted_module"]` test does
    (onnx_optimized_inference.py:74)."""
    from qtx.session import run_module
    feeds = {"global_in": golden_model["enc_in"], "global_in_1": golden_model["src_mask"]}
    p = {"inject_type": "INPUT", "faulty_operation_name": "MatMul_15",
         "targetted_module": "Decoder", "faulty_bit_position": 7}
    outs, wd = run_module("Encoder", feeds, None, {}, None, inject_parameters=p,
                          model=gpu_model, rng=np.random.default_rng(3))
    assert "qtx_fault" not in wd
    ref = oracle_model.encode(golden_model["enc_in"], golden_model["src_mask"])
    np.testing.assert_array_equal(outs["global_out"], ref)


@pytest.mark.gpu
def test_run_module_random_fault_on_foreign_name_is_golden(torch_gpu, gpu_model, oracle_model,
                                                           golden_model):
    """A RANDOM fault names a node alone (onnx_optimized_inference.py:59): on a module whose
    graph has no MatMul of that name (MatMul_60 is a decoder MatMul; the encoder's end at
    MatMul_47) the reference finds nothing to inject and the run is golden."""
    from qtx.session import run_module
    feeds = {"global_in": golden_model["enc_in"], "global_in_1": golden_model["src_mask"]}
    p = {"inject_type": "RANDOM", "faulty_operation_name": "MatMul_60",
         "targetted_module": "Decoder", "faulty_bit_position": 3}
    outs, wd = run_module("Encoder", feeds, None, {}, None, inject_parameters=p,
                          model=gpu_model, rng=np.random.default_rng(3))
    assert "qtx_fault" not in wd
    ref = oracle_model.encode(golden_model["enc_in"], golden_model["src_mask"])
    np.testing.assert_array_equal(outs["global_out"], ref)


ATTN_CASES = [("INPUT", "QK"), ("INPUT16", "QK"), ("WEIGHT", "QK"), ("WEIGHT16", "QK"),
              ("RANDOM", "QK"), ("INPUT", "PV"), ("INPUT16", "PV"), ("WEIGHT", "PV"),
              ("WEIGHT16", "PV"), ("RANDOM", "PV")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,linear", ATTN_CASES)
def test_encoder_attention_fault_matches_oracle(torch_gpu, gpu_model, oracle_model, kind, linear):
    torch = torch_gpu
    B, S = 3, 24
    src, m, x = _enc_inputs(oracle_model, B, S, 21)
    rng = np.random.default_rng(abs(hash((kind, linear))) % 2**32)
    f = F.random_attn_fault(rng, kind, 0, int(rng.integers(6)), linear, B, S, S, bit=7)
    if kind == "RANDOM":
        f.value = 37.25
    out = gpu_model.encode(torch.from_numpy(x).cuda(),
                           torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda(),
                           fault=f).cpu().numpy()
    np.testing.assert_array_equal(out, oracle_model.encode(x, m, fault=f.as_dict()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,linear", [("INPUT", "CQK"), ("WEIGHT16", "CPV"), ("RANDOM", "CPV"),
                                         ("WEIGHT", "QK"), ("INPUT16", "PV")])
def test_decoder_attention_fault_matches_oracle(torch_gpu, gpu_model, oracle_model, kind, linear):
    torch = torch_gpu
    B, S, T = 2, 20, 6
    src, m, x = _enc_inputs(oracle_model, B, S, 22)
    rng = np.random.default_rng(8)
    memory = oracle_model.encode(x, m)
    y = oracle_model.embed(rng.integers(4, 4444, (B, T)), oracle_model.tgt_lut)
    tm = np.tril(np.ones((1, T, T), np.uint8))
    Sk = S if linear.startswith("C") else T
    f = F.random_attn_fault(rng, kind, 1, int(rng.integers(6)), linear, B, T, Sk, bit=6)
    if kind == "RANDOM":
        f.value = -9.5
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = gpu_model.decode(T_(y), T_(memory), T_(m.reshape(B, S).astype(np.uint8)),
                           T_(tm[0]), fault=f).cpu().numpy()
    np.testing.assert_array_equal(out, oracle_model.decode(y, memory, m, tm, fault=f.as_dict()))


def test_oracle_attention_fault_semantics():
    """Oracle attention with a QK^T INPUT fault over all keys == attention on the flipped q."""
    rng = np.random.default_rng(4)
    B, S = 2, 9
    q, k, v = (rng.integers(-127, 128, (B, S, 512)).astype(np.int8) for _ in range(3))
    sq, sk, sv = (rng.uniform(0.002, 0.03, (B, S)).astype(f32) for _ in range(3))
    mask = np.ones((B, 1, S), np.uint8)
    q2 = q.copy()
    q2[1, 4, 3 * 64 + 10] = O._flip8(q2[1, 4, 3 * 64 + 10], 7)
    want, _ = O.attention(q2, sq, k, sk, v, sv, mask)
    got, _ = O.attention(q, sq, k, sk, v, sv, mask, fault=dict(
        kind="QK_INPUT", b=1, h=3, i=4, j=0, d=10, lo=0, hi=S, bit=7, value=0.0))
    np.testing.assert_array_equal(got, want)
    v2 = v.copy()
    v2[0, 5, 2 * 64 + 7] = O._flip8(v2[0, 5, 2 * 64 + 7], 6)
    want, _ = O.attention(q, sq, k, sk, v2, sv, mask)
    got, _ = O.attention(q, sq, k, sk, v, sv, mask, fault=dict(
        kind="PV_WEIGHT", b=0, h=2, i=0, j=5, d=7, lo=0, hi=S, bit=6, value=0.0))
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,linear,step", [("INPUT", "FFN1", 1), ("WEIGHT", "CPV", 3),
                                              ("RANDOM", "QK", 2)])
def test_greedy_decode_with_decoder_fault(torch_gpu, gpu_model, oracle_model, kind, linear, step):
    """The reference campaign's decode loop with a decoder fault at one step
    (target_inference_number), full-prefix recompute per step, == the oracle."""
    from qtx.decode import greedy_decode_fault
    B, S, L = 2, 14, 8
    src, m, _ = _enc_inputs(oracle_model, B, S, 31)
    rng = np.random.default_rng(9)
    T = step                                       # prefix length of the faulty step
    if linear in F.ATTN:
        f = F.random_attn_fault(rng, kind, 1, 3, linear, B, T, S if linear[0] == "C" else T, bit=7)
    else:
        f = F.random_fault(rng, kind, 1, 3, linear, B * T, bit=7)
    if kind == "RANDOM":
        f.value = 1e4
    ys = greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, target_inference_number=step)
    ref = oracle_model.greedy_decode(src, m, max_len=L, fault=f.as_dict(), fault_step=step - 1)
    np.testing.assert_array_equal(ys, ref)


# ------------------------------------------------------------------ edge coordinates (GPU)
# Explicit faults at the coordinates where an index computation can go wrong: the first and
# last row of a 128-row tile, a ragged last tile, windows that straddle a tile or end at the
# last row, the first / last column, the first / last weight row of each linear of a
# concatenated GEMM (Q|K|V, CK|CV), operands that hold the extreme code, keys past 64.
# Encoder B, S = 3, 50 (150 rows: tiles of 128 + 22); decoder B, T, S = 3, 45, 70 (135 token
# rows: 128 + 7; 210 memory rows: 128 + 82).  Sentence 1 is padded (20 / 30 tokens).
_EDGE = {}
E_B, E_S = 3, 50
D_B, D_T, D_S = 3, 45, 70
ENC_LIN = ("Q", "K", "V", "O", "FFN1", "FFN2")
DEC_LIN = ("Q", "K", "V", "O", "CQ", "CK", "CV", "CO", "FFN1", "FFN2")
KINDS = ("INPUT", "WEIGHT", "INPUT16", "WEIGHT16", "RANDOM")


def _memo(key, fn):
    if key not in _EDGE:
        _EDGE[key] = fn()
    return _EDGE[key]


def _src(B, S, lens, seed):
    rng = np.random.default_rng(seed)
    src = np.full((B, S), 2, np.int64)
    for b, n in enumerate(lens):
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
    return src, (src != 2)[:, None, :]


def _edge_enc(om):
    """(src, mask, x, golden memory) of the encoder edge cases; row 90 is a padded token."""
    def make():
        src, m = _src(E_B, E_S, (50, 20, 50), 51)
        x = om.embed(src, om.src_lut)
        return src, m, x, om.encode(x, m)
    return _memo("enc", make)


def _edge_dec(om):
    """(memory mask, memory, y, tgt mask, golden output) of the decoder edge cases."""
    def make():
        src, m = _src(D_B, D_S, (70, 30, 70), 52)
        memory = om.encode(om.embed(src, om.src_lut), m)
        ys = np.random.default_rng(53).integers(4, 4444, (D_B, D_T))
        y = om.embed(ys, om.tgt_lut)
        tm = np.tril(np.ones((1, D_T, D_T), np.uint8))
        return m, memory, y, tm, om.decode(y, memory, m, tm)
    return _memo("dec", make)


def _linear_edge_faults(module, linears, rows_of):
    """One explicit fault per (linear, kind) pair and per edge coordinate; rows_of(linear):
    the token rows of the linear's input (memory rows for CK / CV)."""
    out = []
    for li, lin in enumerate(linears):
        N, K = F.linear_shape(lin)
        M = rows_of(lin)
        layer = li % 6
        edge = (0, 127, 128, M - 1)
        cols = (0, K - 1)
        mk = lambda kind, **kw: F.Fault(kind, module, layer, lin, **kw)
        out.append(mk("INPUT", row=edge[li % 4], col=cols[li % 2], bit=7))
        out.append(mk("INPUT", row=edge[(li + 2) % 4], col=cols[(li + 1) % 2], bit=6))
        for wr in (0, N - 1):      # Q|K|V and CK|CV: the off + row arithmetic of fault_for
            out.append(mk("WEIGHT", row=wr, col=cols[(li + (wr > 0)) % 2], bit=7))
        starts = (0, N - 16, 505) if lin == "FFN1" else (0, N - 16)
        for k, ws in enumerate(starts):
            out.append(mk("INPUT16", row=edge[(li + k + 1) % 4], col=(37 * li + 5) % K, bit=7,
                          win_start=ws, win_len=16))
        for k, (ws, wl) in enumerate(((120, min(16, M - 120)), (M - 3, 3))):   # over the tile edge
            out.append(mk("WEIGHT16", row=(N - 1, 0)[k], col=(91 * li + 3) % K, bit=7,
                          win_start=ws, win_len=wl))
        out.append(mk("RANDOM", row=edge[(li + 3) % 4], col=(0, N - 1)[li % 2], value=50.0))
    return out


ENC_EDGE = _linear_edge_faults(0, ENC_LIN, lambda lin: E_B * E_S)
# a fault row that is a padded token (sentence 1 holds 20 tokens: row 90 is padding)
ENC_EDGE += [F.Fault("INPUT", 0, 3, "O", row=90, col=17, bit=7),
             F.Fault("RANDOM", 0, 1, "FFN2", row=90, col=3, value=-8.0)]
DEC_EDGE = _linear_edge_faults(1, DEC_LIN,
                               lambda lin: D_B * (D_S if lin in ("CK", "CV") else D_T))
DEC_EDGE += [F.Fault("INPUT", 1, 2, "CK", row=70 + 55, col=9, bit=7)]      # a padded memory row


def _fid(f):
    return (f"{f.linear}-{f.kind}-L{f.layer}-r{f.row}-c{f.col}" +
            (f"-w{f.win_start}+{f.win_len}" if f.win_len else "") +
            (f"-v{f.value:g}" if f.kind == "RANDOM" else f"-b{f.bit}"))


def test_edge_cases_cover_every_linear_and_kind():
    for cases, linears in ((ENC_EDGE, ENC_LIN), (DEC_EDGE, DEC_LIN)):
        assert {(f.linear, f.kind) for f in cases} >= {(l, k) for l in linears for k in KINDS}
        for lin in ("Q", "K", "V") + (("CK", "CV") if linears is DEC_LIN else ()):
            assert {f.row for f in cases if f.linear == lin and f.kind == "WEIGHT"} >= {0, 511}


def _enc_run(torch, gpu_model, om, f):
    src, m, x, gold = _edge_enc(om)
    out = gpu_model.encode(torch.from_numpy(x).cuda(),
                           torch.from_numpy(m.reshape(E_B, E_S).astype(np.uint8)).cuda(),
                           fault=f).cpu().numpy()
    ref = om.encode(x, m, fault=f.as_dict())
    np.testing.assert_array_equal(out, ref)
    return ref, gold


def _dec_run(torch, gpu_model, om, f):
    m, memory, y, tm, gold = _edge_dec(om)
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = gpu_model.decode(T_(y), T_(memory), T_(m.reshape(D_B, D_S).astype(np.uint8)),
                           T_(tm[0]), fault=f).cpu().numpy()
    ref = om.decode(y, memory, m, tm, fault=f.as_dict())
    np.testing.assert_array_equal(out, ref)
    return ref, gold


@pytest.mark.gpu
@pytest.mark.parametrize("f", ENC_EDGE, ids=_fid)
def test_encoder_fault_edges(torch_gpu, gpu_model, oracle_model, f):
    ref, gold = _enc_run(torch_gpu, gpu_model, oracle_model, f)
    if f.kind in ("INPUT", "RANDOM"):        # a whole-row perturbation is never a golden run
        assert not np.array_equal(ref, gold)


@pytest.mark.gpu
@pytest.mark.parametrize("f", DEC_EDGE, ids=_fid)
def test_decoder_fault_edges(torch_gpu, gpu_model, oracle_model, f):
    ref, gold = _dec_run(torch_gpu, gpu_model, oracle_model, f)
    # a perturbed row of a linear that writes the residual stream is never a golden run (one
    # behind an attention can be: a single causal key, a P code that does not move)
    if f.kind in ("INPUT", "RANDOM") and f.linear in ("O", "CO", "FFN1", "FFN2"):
        assert not np.array_equal(ref, gold)


@pytest.mark.gpu
def test_fault_on_extreme_codes(torch_gpu, gpu_model, oracle_model):
    """Operands that store an extreme code, searched on the oracle side in layer 0's Q
    input and Q weight.  The symmetric quantizer stores no -128, and in these inputs every
    row of the Q input has its extreme at -127 (none holds 127); the weight holds both.
    Input -127: bit 7 gives 1, bit 0 gives -128 (the one way a -128 operand arises).
    Weight 127: bit 7 gives -1, bit 0 gives 126."""
    om = oracle_model
    src, m, x, gold = _edge_enc(om)
    qx, _ = O.quant_rows(O.layer_norm(x, *om.enc[0]["ln"][0]).reshape(-1, 512))
    qw = om.enc[0]["attn"][0].q
    assert not (qx == -128).any() and not (qx == 127).any() and not (qw == -128).any()
    r, c = np.argwhere(qx == -127)[-1]                  # the last one: a row of the ragged tile
    wr, wc = np.argwhere(qw == 127)[0]
    assert r >= 128
    for f in (F.Fault("INPUT", 0, 0, "Q", row=int(r), col=int(c), bit=7),
              F.Fault("INPUT", 0, 0, "Q", row=int(r), col=int(c), bit=0),
              F.Fault("WEIGHT", 0, 0, "Q", row=int(wr), col=int(wc), bit=7),
              F.Fault("WEIGHT", 0, 0, "Q", row=int(wr), col=int(wc), bit=0)):
        ref, _ = _enc_run(torch_gpu, gpu_model, om, f)
        assert not np.array_equal(ref, gold)


# RANDOM values whose squared deviation overflows fp32 in the LayerNorm that follows the
# O projection / FFN2 (the reference draws such values in about a quarter of its RANDOM
# faults: delta_init takes a uniform 32-bit pattern).  FFN2 of layer 0 feeds the next layer's
# LayerNorm + quantizer, FFN2 of layer 5 the stack's final norm (fp32 out).
LN_RANDOM = [(lin, layer, v) for lin, layer in (("O", 2), ("FFN2", 0), ("FFN2", 5))
             for v in (1e20, -1e30)]


@pytest.mark.gpu
@pytest.mark.parametrize("module", [0, 1], ids=["enc", "dec"])
@pytest.mark.parametrize("linear,layer,value", LN_RANDOM)
def test_random_fault_overflows_layernorm_variance(torch_gpu, gpu_model, oracle_model, module,
                                                   linear, layer, value):
    """Precondition (CPU): the oracle's output is finite — the variance is +inf, the
    divisor +inf, every element of the row (a_2 * d) / inf + b_2 = b_2.  Holds for both
    values on every case here, so none had to be lowered."""
    rows = E_B * E_S if module == 0 else D_B * D_T
    f = F.Fault("RANDOM", module, layer, linear, row=rows - 1, col=511, value=value)
    ref, gold = (_enc_run if module == 0 else _dec_run)(torch_gpu, gpu_model, oracle_model, f)
    assert np.isfinite(ref).all()
    assert not np.array_equal(ref, gold)


# ---- attention kinds at the edges (decoder, T = 45 queries, S = 70 memory keys) --------
def _dec_self_p_codes(om):
    """P codes [B, H, T, T] of decoder layer 0's self-attention (oracle side)."""
    def make():
        _, _, y, tm, _ = _edge_dec(om)
        lin = om.dec[0]["self_attn"]
        h = O.layer_norm(y, *om.dec[0]["ln"][0])
        (qq, sq), (qk, sk), (qv, sv) = (lin[i](h, quantize_output=True) for i in range(3))
        return O.attention(qq, sq, qk, sk, qv, sv, np.broadcast_to(tm, (D_B, D_T, D_T)), om.H,
                           dec=True)[1]
    return _memo("pcodes", make)


ATTN_EDGE = [
    # a key j >= 64 (the second 64-key block of k_attn_fault_rows), every kind
    ("key66-CQK-WEIGHT", F.Fault("WEIGHT", 1, 1, "CQK", row=0 * D_S + 66, col=3 * 64 + 5, bit=7), False),
    ("key69-CPV-WEIGHT", F.Fault("WEIGHT", 1, 4, "CPV", row=2 * D_S + 69, col=7 * 64 + 63, bit=7), False),
    ("key65-CPV-INPUT", F.Fault("INPUT", 1, 0, "CPV", row=2 * D_T + 44, col=2 * D_S + 65, bit=7), False),
    ("keys54-70-CQK-INPUT16", F.Fault("INPUT16", 1, 5, "CQK", row=0 * D_T + 30, col=64, bit=7,
                                    win_start=54, win_len=16), False),
    ("key68-CQK-RANDOM", F.Fault("RANDOM", 1, 2, "CQK", row=2 * D_T + 1, col=5 * D_S + 68, value=400.0), False),
    # a masked key (sentence 1: 30 memory tokens, keys 30 .. 69 are padding): a golden run
    ("masked-CQK-WEIGHT", F.Fault("WEIGHT", 1, 3, "CQK", row=1 * D_S + 50, col=100, bit=7), True),
    ("masked-CPV-WEIGHT", F.Fault("WEIGHT", 1, 3, "CPV", row=1 * D_S + 67, col=100, bit=7), True),
    ("masked-CQK-RANDOM", F.Fault("RANDOM", 1, 0, "CQK", row=1 * D_T + 7, col=4 * D_S + 64, value=1e30), True),
    # WEIGHT16 window [T - 2, T)
    ("lastrows-QK-WEIGHT16", F.Fault("WEIGHT16", 1, 1, "QK", row=1 * D_T + 10, col=6 * 64 + 1, bit=7,
                                   win_start=D_T - 2, win_len=2), False),
    ("lastrows-CPV-WEIGHT16", F.Fault("WEIGHT16", 1, 5, "CPV", row=0 * D_S + 64, col=1 * 64, bit=6,
                                    win_start=D_T - 2, win_len=2), False),
    # QK RANDOM with a huge value of either sign
    ("QK-RANDOM+1e30", F.Fault("RANDOM", 1, 2, "QK", row=2 * D_T + 44, col=0 * D_T + 17, value=1e30), False),
    ("QK-RANDOM-1e30", F.Fault("RANDOM", 1, 2, "QK", row=2 * D_T + 44, col=7 * D_T + 44, value=-1e30), False),
    ("CQK-RANDOM-1e30", F.Fault("RANDOM", 1, 4, "CQK", row=0 * D_T + 0, col=3 * D_S + 69, value=-1e30), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,f,golden", ATTN_EDGE, ids=[c[0] for c in ATTN_EDGE])
def test_decoder_attention_fault_edges(torch_gpu, gpu_model, oracle_model, name, f, golden):
    ref, gold = _dec_run(torch_gpu, gpu_model, oracle_model, f)
    assert np.isfinite(ref).all()
    assert np.array_equal(ref, gold) == golden        # the oracle itself: a masked key changes nothing


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["zero", "largest"])
def test_pv_input_fault_on_zero_and_largest_code(torch_gpu, gpu_model, oracle_model, which):
    """PV INPUT, bit 7: on a P code of 0 (a causally masked key: 0 -> -128) and on the
    row's largest code (found in the oracle's P of layer 0)."""
    qp = _dec_self_p_codes(oracle_model)
    b, h, i = 2, 5, 40
    if which == "zero":
        j = 44                                         # j > i: masked, code 0
        assert qp[b, h, i, j] == 0
    else:
        j = int(np.argmax(qp[b, h, i]))
        assert qp[b, h, i, j] >= 8 and j <= i
    f = F.Fault("INPUT", 1, 0, "PV", row=b * D_T + i, col=h * D_T + j, bit=7)
    ref, gold = _dec_run(torch_gpu, gpu_model, oracle_model, f)
    assert not np.array_equal(ref, gold)


@pytest.mark.gpu
def test_greedy_decode_with_encoder_fault_in_second_tile(torch_gpu, gpu_model, oracle_model):
    torch = torch_gpu
    src, m, _, _ = _edge_enc(oracle_model)
    f = F.Fault("INPUT", 0, 4, "FFN2", row=141, col=2047, bit=7)
    ids = gpu_model.greedy(torch.from_numpy(src).cuda(),
                           torch.from_numpy(m.reshape(E_B, E_S).astype(np.uint8)).cuda(),
                           max_len=9, fault=f).cpu().numpy()
    ref = oracle_model.greedy_decode(src, m, max_len=9, fault=f.as_dict())
    np.testing.assert_array_equal(ids, ref)
    # the fault row belongs to sentence 2: the other sentences decode as in a golden run
    np.testing.assert_array_equal(ref[:2], oracle_model.greedy_decode(src[:2], m[:2], max_len=9))
