"""Every exported entry point that takes a device pointer, with every pointer at the least
alignment include/qtx.h promises to accept: 16 (mod 256).

tests/test_gpu_bounds.py runs the kernel-level entries (and the plain encoder, decoder and
greedy calls) at that alignment through its `gb` fixture.  This module covers the rest of the
header: each case below makes one call — or one home test's worth of calls — with all device
pointers and the workspace at 16 (mod 256) and compares with the reference its home test
file uses (score_ref, beam_ref, kvfault_ref, kvtrials_ref, dfault_cases, model_cfgs, with
their memoised oracle results).  COVERED / EXEMPT below and the entries test_gpu_bounds.py
calls must account for every function of the header that has a pointer parameter
(test_every_pointer_entry_is_accounted_for, on the CPU).

How the pointers get there (the `skew` fixture).  The Python layer and the home tests turn a
tensor into a pointer in one place each (qtx.model._ptr, a test module's P); the fixture
replaces those with Skew.ptr, which hands out the address of a twin: a copy of the tensor's
whole storage at 16 (mod 256), kept for the length of the test (a workspace keeps its
address between a decode and its resume).  The library itself sits behind a proxy that, on
every call, checks that each device pointer it receives lies inside a twin (so no pointer of
the call can have kept its 256-byte alignment), copies the originals into the twins, calls,
and copies the twins back.  A workspace at 16 (mod 256) puts every sub-buffer the carve hands
out (csrc/qtx_carve.h rounds offsets, not addresses) at 16 (mod 256) as well.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import dfault_cases as D  # noqa: E402
import long_target as LT  # noqa: E402
import model_cfgs as MC  # noqa: E402
import score_ref as SR  # noqa: E402
from guarded import skewed  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
S0 = C.c_void_p(0)
SKEW = 16
KEY97 = (512, 8, 97)            # the two-layer d_ff 512 model of 97 words
GR = (3, 13, 23)                # B, S, max_len of the model-level cases

# entry -> the test of this module that calls it at 16 (mod 256)
COVERED = {
    "qtx_model_create": "test_model_create_then_encode",
    "qtx_encoder_forward_fault": "test_encoder_and_decoder_forward_fault",
    "qtx_decoder_forward_fault": "test_encoder_and_decoder_forward_fault",
    "qtx_greedy_decode_fault": "test_greedy_decode_fault",
    "qtx_greedy_decode_scored": "test_greedy_decode_scored",
    "qtx_greedy_decode_dfault": "test_dfault_and_resume",
    "qtx_greedy_dfault_resume": "test_dfault_and_resume",
    "qtx_greedy_decode_kvfault": "test_kvfault",
    "qtx_greedy_decode_kvtrials": "test_kvtrials",
    "qtx_beam_decode": "test_beam_decode",
    "qtx_score_targets": "test_score_targets",
    "qtx_score_logits": "test_score_logits",
    "qtx_score_rows": "test_score_rows",
    "qtx_generator_top2": "test_generator_top2",
    "qtx_decode_top2_embed": "test_decode_top2_embed",
    "qtx_decode_generator": "test_decode_generator",
    "qtx_beam_select": "test_beam_select",
    "qtx_beam_reorder": "test_beam_reorder",
    "qtx_linear_i8_rowfaults": "test_linear_i8_rowfaults",
}
# entries with a pointer parameter that no alignment case can say anything about
EXEMPT = {
    "qtx_model_tensor_count": "query: reads a host qtx_config",
    "qtx_model_destroy": "takes the model handle only",
    "qtx_model_device_bytes": "query on the model handle",
    "qtx_model_linear": "query: returns the model's own device pointers through host pointers",
    "qtx_model_norm": "query: returns the model's own device pointers through host pointers",
    "qtx_encoder_workspace_size": "query on the model handle",
    "qtx_decoder_workspace_size": "query on the model handle",
    "qtx_greedy_workspace_size": "query on the model handle",
    "qtx_greedy_scored_workspace_size": "query on the model handle",
    "qtx_greedy_dfault_workspace_size": "query on the model handle",
    "qtx_greedy_kvfault_workspace_size": "query on the model handle",
    "qtx_greedy_kvtrials_workspace_size": "query on the model handle",
    "qtx_beam_workspace_size": "query on the model handle",
    "qtx_score_workspace_size": "query on the model handle",
    "qtx_model_check": "the model handle and a stream; reads the model's own status word",
    "qtx_debug_nop": "debug: a stream and no buffer",
    "qtx_debug_graph_stats": "debug: the model handle and host pointers",
}


# =====================================================================================
# the header's functions and who covers them (CPU)
# =====================================================================================
def header_functions():
    """{name: parameter list text} of every function include/qtx.h declares."""
    text = open(os.path.join(REPO, "include", "qtx.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decl = re.findall(r"\b(?:const\s+char\s*\*|int32_t|int64_t|size_t|void)\s+(qtx_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;",
                      text, flags=re.S)
    return {name: " ".join(params.split()) for name, params in decl}


def bounds_entries():
    """The entry points tests/test_gpu_bounds.py calls (at both alignments, through `gb`)."""
    text = open(os.path.join(REPO, "tests", "test_gpu_bounds.py")).read()
    return set(re.findall(r"\b(qtx_[a-z0-9_]+)\b", text))


def test_every_pointer_entry_is_accounted_for():
    fns = header_functions()
    from qtx import _lib
    assert set(fns) == set(_lib.header_symbols()) and len(fns) > 50
    assert fns["qtx_debug_reload_knobs"] == "void" and "const float* pe" in fns["qtx_model_create"]
    with_ptr = {n for n, p in fns.items() if "*" in p}
    bounds = bounds_entries() & set(fns)
    assert {"qtx_linear_rows", "qtx_skinny_linear", "qtx_greedy_decode", "qtx_embed"} <= bounds
    missing = sorted(with_ptr - bounds - set(COVERED) - set(EXEMPT))
    assert not missing, f"no minimum-alignment case and no exemption for {missing}"
    # the tables name real functions and real tests, and exempt nothing that has a case
    assert set(COVERED) <= with_ptr and set(EXEMPT) <= with_ptr
    assert not set(EXEMPT) & set(COVERED)
    assert all(callable(globals().get(t)) for t in COVERED.values())
    assert all(EXEMPT.values())


# =====================================================================================
# the skew fixture
# =====================================================================================
pytest_gpu = pytest.mark.gpu      # (not a module-wide pytestmark: the test above runs on the CPU)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Skew:
    """Twins at 16 (mod 256) of the storages whose pointers pass through ptr()."""

    def __init__(self, torch):
        self.torch, self.twins, self.called = torch, {}, []
        self.fns = header_functions()

    def ptr(self, t):
        if t is None:
            return C.c_void_p(0)
        torch = self.torch
        st = t.untyped_storage()
        key = st.data_ptr()
        if key not in self.twins:
            n = st.nbytes()
            flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,))
            buf = torch.empty(n + 512, dtype=torch.uint8, device=t.device)
            off = (-buf.data_ptr()) % 256 + SKEW
            twin = buf[off:off + n]
            assert twin.data_ptr() % 256 == SKEW
            twin.copy_(flat)
            self.twins[key] = (flat, twin)
        twin = self.twins[key][1]
        return C.c_void_p(twin.data_ptr() + t.data_ptr() - key)

    def _inside(self, addr):
        return any(tw.data_ptr() <= addr < tw.data_ptr() + max(tw.numel(), 1)
                   for _, tw in self.twins.values())

    def run(self, name, fn, args):
        params = self.fns.get(name, "")
        if "*" not in params or name in EXEMPT:
            return fn(*args)
        for i, a in enumerate(args):
            if isinstance(a, C.c_void_p) and a.value:
                if i == 0 and params.startswith("const qtx_model*"):
                    continue                          # the handle
                # (a pointer made outside ptr(), as qtx_model_create's, must be at 16 itself)
                assert self._inside(a.value) or a.value % 256 == SKEW, \
                    f"{name}: argument {i} is a device pointer that is not at 16 (mod 256)"
        for flat, twin in self.twins.values():
            twin.copy_(flat)
        rc = fn(*args)
        for flat, twin in self.twins.values():
            flat.copy_(twin)
        self.called.append(name)
        return rc


class _LibProxy:
    def __init__(self, real, skew):
        self._real, self._skew = real, skew

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("qtx_"):
            return fn
        return lambda *args: self._skew.run(name, fn, args)


def _home_modules():
    import test_gpu_beam
    import test_gpu_bounds
    import test_gpu_dfault_cached
    import test_gpu_kvfault
    import test_gpu_kvtrials
    import test_gpu_rowfault_gemm
    import test_gpu_score
    import test_gpu_scored
    return (test_gpu_beam, test_gpu_bounds, test_gpu_dfault_cached, test_gpu_kvfault,
            test_gpu_kvtrials, test_gpu_rowfault_gemm, test_gpu_score, test_gpu_scored)


@pytest.fixture
def skew(torch, monkeypatch):
    from qtx import _lib, model
    s = Skew(torch)
    monkeypatch.setattr(_lib, "_lib", _LibProxy(_lib.lib(), s))
    monkeypatch.setattr(model, "_ptr", s.ptr)
    for mod in _home_modules():
        monkeypatch.setattr(mod, "P", s.ptr)
    yield s
    torch.cuda.synchronize()


def make_model_skewed(torch, sd, cfg):
    """A QtxModel whose qtx_model_create saw every fp32 tensor and the positional table at
    16 (mod 256) (QtxModel.__init__ with the uploads replaced)."""
    import threading

    from qtx import _lib
    from qtx.model import QtxModel, _stream
    from qtx.weights import positional_table, tensor_order
    gm = QtxModel.__new__(QtxModel)
    gm.cfg = cfg
    gm.device = torch.device("cuda", torch.cuda.current_device())
    gm.ccfg = _lib.QtxConfig(cfg.src_vocab, cfg.tgt_vocab, cfg.n_layers, cfg.d_model, cfg.d_ff,
                             cfg.n_heads, cfg.max_len, cfg.weight_bits)
    keys = tensor_order(cfg)
    assert _lib.lib().qtx_model_tensor_count(C.byref(gm.ccfg)) == len(keys)
    dev = [skewed(torch, np.ascontiguousarray(sd[k], f32).reshape(-1), SKEW) for k in keys]
    pe_np = sd.get("src_embed.1.pe")
    pe_np = positional_table(cfg.d_model, cfg.max_len) if pe_np is None else pe_np
    pe = skewed(torch, np.ascontiguousarray(pe_np, f32).reshape(-1), SKEW)
    assert all(t.data_ptr() % 256 == SKEW for t in dev + [pe])
    arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    h = C.c_void_p()
    _lib.call("qtx_model_create", C.byref(gm.ccfg), arr, len(dev), C.c_void_p(pe.data_ptr()),
              _stream(gm.device), C.byref(h))
    gm.handle = h
    gm._tls = threading.local()
    _CREATED.append("qtx_model_create")
    return gm


_MODELS = {}
_CREATED = []       # "qtx_model_create" once a model of this module has been created



def model_of(torch, key, pe_rows=None):
    """(QtxModel created from tensors at 16 (mod 256), OracleModel) of one small config."""
    k = (key, pe_rows)
    if k not in _MODELS:
        cfg, sd, om = MC.small_state(*key) if pe_rows is None else LT.state(key[0], key[1], pe_rows)
        _MODELS[k] = (make_model_skewed(torch, sd, cfg), om)
    return _MODELS[k]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _MODELS.clear()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


# =====================================================================================
# model creation, the plain model calls on every chain, the switches of the decode
# =====================================================================================
@pytest_gpu
def test_model_create_then_encode(torch, skew):
    """qtx_model_create from tensors and a positional table at 16 (mod 256), then one encode,
    one decoder pass and one greedy decode with every pointer there: == the oracle."""
    import test_gpu_model_configs as TMC
    gm, om = model_of(torch, KEY97)
    TMC.check_model(torch, gm, om, KEY97)
    assert {"qtx_model_create", "qtx_encoder_forward", "qtx_decoder_forward",
            "qtx_greedy_decode"} <= set(skew.called) | set(_CREATED)


@pytest_gpu
@pytest.mark.parametrize("env", [{}, {"QTX_DECODE_GROUPS": 2}, {"QTX_UNFUSED": 1}],
                         ids=["default", "groups2", "unfused"])
def test_greedy_decode_paths(torch, skew, knob_env, env):
    """B = 3, S = 13, max_len = 23 on the two-layer d_ff 512 model: the fused step, two
    sub-batch graphs (the carve hands each group its own scratch) and the unfused step."""
    import test_gpu_model_configs as TMC
    for k, v in env.items():
        knob_env(k, v)
    gm, om = model_of(torch, KEY97)
    src, m, ys, _, _ = TMC.greedy_case(KEY97, om, *GR)
    np.testing.assert_array_equal(TMC.gpu_greedy(gm, src, m, GR[2]), ys)
    assert "qtx_greedy_decode" in skew.called


@pytest_gpu
@pytest.mark.parametrize("key", [(256, 8, 97), (512, 4, 97)], ids=["dff256", "int4"])
def test_generic_chain_and_int4(torch, skew, key):
    """d_ff 256 (the generic chain: k_gemm, the unfused step) and 4-bit weights (packed at
    creation from tensors at 16 (mod 256)): encode and greedy."""
    import test_gpu_model_configs as TMC
    gm, om = model_of(torch, key)
    x, m, memory = TMC.enc_case(key, om)
    np.testing.assert_array_equal(TMC.gpu_encode(torch, gm, x, m), memory)
    src, sm, ys, _, _ = TMC.greedy_case(key, om, *GR)
    np.testing.assert_array_equal(TMC.gpu_greedy(gm, src, sm, GR[2]), ys)
    assert {"qtx_encoder_forward", "qtx_greedy_decode"} <= set(skew.called)


@pytest_gpu
def test_greedy_decode_140_positions(torch, skew):
    """max_len 140 on the 192-row-table model of tests/long_target.py: the carve for more than
    128 positions, the unfused step and the generic attention kernel."""
    from qtx.decode import greedy_decode
    c = (512, 8)
    gm, _ = model_of(torch, c, LT.PE_ROWS)
    src, m = LT.inputs()
    oy, _, _ = LT.scored(c)
    np.testing.assert_array_equal(greedy_decode(gm, src, m, LT.L, 0), oy)
    assert "qtx_greedy_decode" in skew.called


# =====================================================================================
# the fault forms of the model calls
# =====================================================================================
@pytest_gpu
def test_encoder_and_decoder_forward_fault(torch, skew):
    import test_gpu_model_configs as TMC
    gm, om = model_of(torch, KEY97)
    x, m, memory = TMC.enc_case(KEY97, om)
    f = TMC.ffn_faults(512, 0, TMC.ENC_B * TMC.ENC_S)[3]          # INPUT, FFN2, bit 7
    ref = TMC.memo(("ffault", KEY97, 0, 3), lambda: om.encode(x, m, fault=f.as_dict()))
    assert not np.array_equal(ref, memory)
    np.testing.assert_array_equal(TMC.gpu_encode(torch, gm, x, m, fault=f), ref)
    y, tm, gold = TMC.dec_case(KEY97, om)
    f = TMC.ffn_faults(512, 1, TMC.ENC_B * TMC.DEC_T)[1]          # WEIGHT, FFN1, bit 6
    ref = TMC.memo(("ffault", KEY97, 1, 1), lambda: om.decode(y, memory, m, tm, fault=f.as_dict()))
    assert not np.array_equal(ref, gold)
    np.testing.assert_array_equal(TMC.gpu_decode(torch, gm, y, memory, m, tm, fault=f), ref)
    assert {"qtx_encoder_forward_fault", "qtx_decoder_forward_fault"} <= set(skew.called)


def _enc_fault():
    from qtx.fault import Fault
    return Fault("WEIGHT", 0, 1, "FFN2", row=300, col=100, bit=7)


@pytest_gpu
def test_greedy_decode_fault(torch, skew):
    """An encoder fault carried through the whole KV-cached decode."""
    import test_gpu_model_configs as TMC
    import test_gpu_scored as TS
    from qtx.decode import greedy_decode_fault
    gm, om = model_of(torch, KEY97)
    src, m, gold, _, _ = TMC.greedy_case(KEY97, om, *GR)
    f = _enc_fault()
    ys, _, _ = TMC.memo(("min-align-encfault", GR),
                        lambda: TS.oracle_scored_decode(om, src, m, GR[2], fault=f.as_dict()))
    assert (ys != gold).sum() >= 3                     # the fault reaches the tokens
    np.testing.assert_array_equal(greedy_decode_fault(gm, src, m, GR[2], 0, fault=f), ys)
    assert "qtx_greedy_decode_fault" in skew.called


@pytest_gpu
def test_greedy_decode_scored(torch, skew):
    import test_gpu_model_configs as TMC
    import test_gpu_scored as TS
    gm, om = model_of(torch, KEY97)
    src, m, ys, ti, tv = TMC.greedy_case(KEY97, om, *GR)
    gy, gi, gv = TS.gpu_scored(gm, src, m, GR[2])
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(bits(gv), bits(tv))
    assert "qtx_greedy_decode_scored" in skew.called


@pytest_gpu
def test_dfault_and_resume(torch, skew, gpu_model, oracle_model):
    """One scored golden decode and two resumes on the same workspace at 16 (mod 256): a
    token-changing trial and a masked one, each == the oracle's trial."""
    import test_gpu_dfault_cached as TDF
    from qtx import decode_fault_sweep
    src, m = D.make_src()
    t = D.trials()
    names = ["output_ffn2_t2", "input_bit0_t2"]
    exp = {n: TDF.expect(oracle_model, n) for n in names}
    assert D.changed(exp["output_ffn2_t2"]) and not D.changed(exp["input_bit0_t2"])
    res, stats = decode_fault_sweep(gpu_model, src, m, TDF.L, 0, [t[n] for n in names])
    assert stats.n_resumed == 1 and stats.n_skipped == 1
    for n, got in zip(names, res):
        TDF.check_scored(got, exp[n], t[n][1])
    assert skew.called.count("qtx_greedy_decode_dfault") == 1
    assert skew.called.count("qtx_greedy_dfault_resume") == 2
    # and the single call
    TDF.check_scored(TDF.cached(gpu_model, *t["output_ffn2_t2"], True), exp["output_ffn2_t2"],
                     t["output_ffn2_t2"][1])


@pytest_gpu
@pytest.mark.parametrize("name", ["in_v_l2_s2", "up_sv_j3"], ids=["step_fault", "cache_upset"])
def test_kvfault(torch, skew, gpu_model, oracle_model, name):
    import test_gpu_kvfault as TKF
    TKF.check(gpu_model, oracle_model, *TKF.CASES[name])
    assert skew.called.count("qtx_greedy_decode_kvfault") == 2      # scored and plain


@pytest_gpu
def test_kvtrials(torch, skew, gpu_model, oracle_model):
    """Table B of tests/test_gpu_kvtrials.py: upsets of all four caches next to step faults."""
    import test_gpu_kvtrials as TKT
    src, m = TKT.batch()
    TKT.check(gpu_model, oracle_model, src, m, TKT.mixes()["B"])
    assert "qtx_greedy_decode_kvtrials" in skew.called


# =====================================================================================
# beam search and target scoring
# =====================================================================================
@pytest_gpu
def test_beam_decode(torch, skew):
    import test_gpu_beam as TB
    d_ff, wb, V, beam = BR.MODELS[0]
    gm = TB.gpu_model(d_ff, wb, V)
    src, mask = BR.inputs(d_ff, wb, V)
    TB.assert_same(TB.gpu_beam(gm, src, mask, beam), BR.reference(d_ff, wb, V, beam))
    assert "qtx_beam_decode" in skew.called


@pytest_gpu
def test_beam_select(torch, skew):
    import test_gpu_beam as TB
    TB.test_select_op(torch, 97, 4, 3)
    assert "qtx_beam_select" in skew.called


@pytest_gpu
@pytest.mark.parametrize("grouped", [1, 0])
def test_beam_reorder(torch, skew, grouped):
    import test_gpu_beam as TB
    TB.reorder_case(torch, (0, 0, 2, 1), 3, grouped, 0xA5)
    assert "qtx_beam_reorder" in skew.called


@pytest_gpu
def test_score_targets(torch, skew):
    import test_gpu_score as TSC
    gm, _ = model_of(torch, KEY97)
    src, mask = SR.inputs()
    got = TSC.score_call(torch, gm, src, mask, SR.targets(*KEY97))
    TSC.same_ref(got, SR.reference(*KEY97), what="at 16 (mod 256)")
    assert "qtx_score_targets" in skew.called


@pytest_gpu
def test_score_logits(torch, skew):
    import test_gpu_score as TSC
    TSC.test_score_logits_on_crafted_rows(torch, 97, 5, 0xA5)
    assert "qtx_score_logits" in skew.called


@pytest_gpu
def test_score_rows(torch, skew):
    """M = 37 rows through a workspace of exactly 16 rows: chunks of 16, 16 and 5."""
    import test_gpu_score as TSC
    from qtx import _lib
    gm, om = model_of(torch, KEY97)
    M, V = 37, 97
    rng = np.random.default_rng(V)
    x = rng.standard_normal((M, 512)).astype(f32)
    y = rng.integers(0, V, M).astype(np.int64)
    y[3], y[20], y[36] = V, -1, V - 1
    exp = SR.score_logits(om.logits(x), y)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ws = torch.empty(16 * V * 4, dtype=torch.uint8, device="cuda")
    ts, checks = TSC.outputs(torch, (M,), 0xA5)
    _lib.call("qtx_score_rows", gm.handle, skew.ptr(xd), M, skew.ptr(yd), *[skew.ptr(t) for t in ts],
              skew.ptr(ws), ws.numel(), S0)
    torch.cuda.synchronize()
    for c in checks:
        c()
    for g, e, k in zip(TSC.to_np(ts), exp, ("tok_logp", "rank", "top_ids", "top_logp")):
        TSC.same(g, e, k)
    assert "qtx_score_rows" in skew.called


# =====================================================================================
# the decode tail
# =====================================================================================
@pytest_gpu
def test_generator_top2(torch, skew):
    import test_gpu_scored as TS
    gm, om = model_of(torch, KEY97)
    rng = np.random.default_rng(37)
    x = (rng.standard_normal((37, 512)) * np.linspace(0.2, 3, 37)[:, None]).astype(f32)
    want_i, want_v = TS.top2_of(om.generator(x)[0])
    ti, tl = gm.generator_top2(torch.from_numpy(x).cuda())
    np.testing.assert_array_equal(ti.cpu().numpy(), want_i)
    np.testing.assert_array_equal(bits(tl.cpu().numpy()), bits(want_v))
    assert "qtx_generator_top2" in skew.called


@pytest_gpu
def test_decode_top2_embed(torch, skew, gpu_model, oracle_model):
    """The home test's crafted rows at V = 4444 (ties, a logp collision, non-finite rows),
    with qtx_decode_argmax_embed on the same input."""
    import test_gpu_scored as TS
    TS.test_decode_top2_embed(torch, lambda V: gpu_model, oracle_model, 4444, 0xA5)
    assert {"qtx_decode_top2_embed", "qtx_decode_argmax_embed"} <= set(skew.called)


@pytest_gpu
@pytest.mark.parametrize("with_rec", [True, False])
def test_decode_generator(torch, skew, with_rec):
    """M = 17 (a full 16-row block and one row), V = 97: the logits == the oracle's generator
    on the final LayerNorm of x, the strip
    records == tail_fold_ref's restatement, nothing past row M - 1."""
    import tail_fold_ref as TR
    from qtx import _lib
    gm, om = model_of(torch, KEY97)
    M, V = 17, 97
    nstrip = (V + 15) // 16
    x = (np.random.default_rng(100 * V + M).standard_normal((M, 512)) * 3).astype(f32)
    xd = torch.from_numpy(x).cuda()
    logits = torch.full((M + 1, V), -7.0, dtype=torch.float32, device="cuda")
    rec = torch.full((M + 1, nstrip, 4), -7.0, dtype=torch.float32, device="cuda")
    _lib.call("qtx_decode_generator", gm.handle, skew.ptr(xd), M, skew.ptr(logits),
              skew.ptr(rec) if with_rec else None, S0)
    torch.cuda.synchronize()
    lg, rc = logits.cpu().numpy(), rec.cpu().numpy()
    assert (lg[M] == -7.0).all() and (rc[M] == -7.0).all()
    np.testing.assert_array_equal(bits(lg[:M]), bits(om.logits(O.layer_norm(x, *om.dec_norm))))
    if not with_rec:
        assert (rc == -7.0).all()
    else:
        ri = rc.view(np.int32)
        for r in range(M):
            want = TR.strip_records(lg[r])
            got = [(rc[r, s, 0], rc[r, s, 1], int(ri[r, s, 2]), int(ri[r, s, 3]))
                   for s in range(len(want))]
            assert got == want, r
    assert "qtx_decode_generator" in skew.called


# =====================================================================================
# the per-row fault GEMM
# =====================================================================================
@pytest_gpu
def test_linear_i8_rowfaults(torch, skew):
    """M = 33 across the 32-row tile, N = 512, K = 2048, residual: the home test's table."""
    import test_gpu_rowfault_gemm as TRF
    TRF.test_matches_the_restatement(torch, *TRF.SHAPES[2])
    assert {"qtx_linear_i8_rowfaults", "qtx_linear_i8"} <= set(skew.called)


# =====================================================================================
# the Python layer passes a view's address, not its storage's
# =====================================================================================
@pytest_gpu
def test_python_layer_passes_view_addresses(torch):
    """QtxModel.encode and decode.greedy_decode on tensors that are views at a 16-byte
    storage offset (a caller that sub-allocates one arena): == the oracle.  A wrapper that
    passed the storage base would read 16 bytes early."""
    import test_gpu_model_configs as TMC
    from qtx.decode import greedy_decode
    gm, om = model_of(torch, KEY97)
    x, m, memory = TMC.enc_case(KEY97, om)
    B, S, _ = x.shape
    xbuf = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
    xv = xbuf[4:4 + x.size].view(x.shape)
    xv.copy_(torch.from_numpy(x))
    mbuf = torch.full((B * S + 32,), 1, dtype=torch.uint8, device="cuda")
    mv = mbuf[16:16 + B * S].view(B, S)
    mv.copy_(torch.from_numpy(np.ascontiguousarray(m.reshape(B, S)).astype(np.uint8)))
    assert xv.data_ptr() % 256 == 16 and mv.data_ptr() % 256 == 16
    assert xv.is_contiguous() and xv.storage_offset() == 4 and mv.storage_offset() == 16
    np.testing.assert_array_equal(gm.encode(xv, mv).cpu().numpy(), memory)
    gm.check()
    src, sm, ys, _, _ = TMC.greedy_case(KEY97, om, *GR)
    ibuf = torch.full((src.size + 4,), 5, dtype=torch.int64, device="cuda")
    sv = ibuf[2:2 + src.size].view(src.shape)
    sv.copy_(torch.from_numpy(src))
    assert sv.data_ptr() % 256 == 16 and sv.storage_offset() == 2
    got = greedy_decode(gm, sv, torch.from_numpy(sm).cuda(), GR[2], 0)
    assert isinstance(got, torch.Tensor)
    np.testing.assert_array_equal(got.cpu().numpy(), ys)
