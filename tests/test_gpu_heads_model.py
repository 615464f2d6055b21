"""Models with 4 and 16 heads (head widths 128 / 32) through the model-level entries, against
oracle/qtx_oracle.py and tests/beam_ref.py, bit for bit: tests/model_cfgs.py's two-layer
d_ff = 512 model with n_heads set (and a 160-row positional table for the 140-position
decodes).  Fault entries refuse such a model with QTX_E_UNSUPPORTED."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from qtx import fault as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402
import model_cfgs as MC  # noqa: E402
from score_ref import score_ref  # noqa: E402
from test_gpu_model_configs import (ENC_B, ENC_S, GR_L, T_, dec_case, enc_case, gpu_decode,  # noqa: E402
                                    gpu_encode, gpu_greedy, greedy_case, u8)
from test_gpu_scored import gpu_scored  # noqa: E402

pytestmark = pytest.mark.gpu
HEADS = (4, 16)
_MODELS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def model(H):
    """(QtxModel, OracleModel) of the d_ff = 512 small model with H heads, built once."""
    if H not in _MODELS:
        from oracle.qtx_oracle import OracleModel
        from qtx.model import QtxModel
        from qtx.weights import synthetic_state_dict
        cfg = dataclasses.replace(MC.small_cfg(512), n_heads=H, max_len=160)
        sd = synthetic_state_dict(1, cfg, ln_random=True)
        _MODELS[H] = (QtxModel(sd, cfg), OracleModel(sd, n_layers=cfg.n_layers, n_heads=H))
    return _MODELS[H]


def graph_captures(gm):
    from qtx import _lib
    e, n = C.c_int32(0), C.c_int64(0)
    _lib.call("qtx_debug_graph_stats", gm.handle, C.byref(e), C.byref(n))
    return n.value


@pytest.mark.parametrize("H", HEADS)
def test_encoder_decoder_forward(torch, H):
    gm, om = model(H)
    x, m, memory = enc_case(("heads", H), om)
    assert x.shape[:2] == (ENC_B, ENC_S)
    np.testing.assert_array_equal(gpu_encode(torch, gm, x, m), memory)
    y, tm, ref = dec_case(("heads", H), om)
    np.testing.assert_array_equal(gpu_decode(torch, gm, y, memory, m, tm), ref)


@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_UNFUSED": 1}], ids=["default", "nograph", "unfused"])
@pytest.mark.parametrize("H", HEADS)
def test_greedy_and_scored(torch, knob_env, H, env):
    gm, om = model(H)
    src, m, ys, ti, tv = greedy_case(("heads", H), om)
    for k, v in env.items():
        knob_env(k, v)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, GR_L), ys)
    n1 = graph_captures(gm)
    gy, gi, gv = gpu_scored(gm, src, m, GR_L)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)
    if not env:      # the step graphs: captured by the first call, none added by a second
        assert n1 >= 1
        n2 = graph_captures(gm)
        np.testing.assert_array_equal(gpu_greedy(gm, src, m, GR_L), ys)
        np.testing.assert_array_equal(gpu_scored(gm, src, m, GR_L)[0], ys)
        assert graph_captures(gm) == n2


@pytest.mark.parametrize("B,S,L", [(2, 130, 140), (100, 9, 9)], ids=["long", "B100"])
@pytest.mark.parametrize("H", HEADS)
def test_greedy_long_and_wide(torch, H, B, S, L):
    """S = 130 / max_len = 140: both attentions of the step past 128 keys; B = 100: the step's
    kernels for 96 rows and more."""
    gm, om = model(H)
    src, m, ys, ti, tv = greedy_case(("heads", H), om, B=B, S=S, L=L)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, L), ys)
    gy, gi, gv = gpu_scored(gm, src, m, L)
    np.testing.assert_array_equal(gy, ys)
    np.testing.assert_array_equal(gi, ti)
    np.testing.assert_array_equal(gv, tv)


@pytest.mark.parametrize("L", [9, 140], ids=["fused", "unfused-body"])
@pytest.mark.parametrize("H", HEADS)
def test_beam(torch, H, L):
    """Beam 4: max_len 9 on the fused step (k_dec_attn_hd + reorder), 140 on the unfused body
    (k_attention_hd with the device counter: k_dec_attn_beam is 64 columns wide)."""
    from qtx.decode import beam_decode
    gm, om = model(H)
    src, m = MC.small_src(2, 9, 5, full=(0,))
    ref = R.beam_ref(om, src, m, L, 4)
    r = beam_decode(gm, src, m, L, R.START, beam_size=4, eos=R.EOS, pad=R.PAD, n_best=4, early_exit=False)
    np.testing.assert_array_equal(r.hyp_ids, ref["hyp_ids"])
    np.testing.assert_array_equal(r.hyp_len, ref["hyp_len"])
    np.testing.assert_array_equal(r.hyp_score.view(np.int32), ref["hyp_score"].view(np.int32))


@pytest.mark.parametrize("H", HEADS)
def test_score_targets(torch, H):
    from qtx.decode import score_targets
    gm, om = model(H)
    src, m, ys, _, _ = greedy_case(("heads", H), om)
    ref = score_ref(om, src, m, ys)
    got = score_targets(gm, src, m, ys)
    np.testing.assert_array_equal(got.tok_logp, ref["tok_logp"])
    np.testing.assert_array_equal(got.rank, ref["rank"])
    np.testing.assert_array_equal(got.top_ids, ref["top_ids"])
    np.testing.assert_array_equal(got.top_logp, ref["top_logp"])


_DEC = lambda a: (a.h, a.src, a.m, 3, 9, 9, 0)
# entry -> its C arguments; a.o(): a fresh guarded output, a.w: the guarded workspace and its size
REFUSED = {
    "qtx_encoder_forward_fault": lambda a: (a.h, a.x, a.em, 3, 50, a.o(), *a.w, a.fe, None),
    "qtx_decoder_forward_fault": lambda a: (a.h, a.y, a.mem, a.em, a.tm, 0, 3, 6, 50, a.o(), *a.w, a.fd, None),
    "qtx_greedy_decode_fault": lambda a: (*_DEC(a), a.o(), *a.w, a.fe, None),
    "qtx_greedy_decode_scored": lambda a: (*_DEC(a), a.o(), a.o(), a.o(), *a.w, a.fe, None),
    "qtx_greedy_decode_dfault": lambda a: (*_DEC(a), *a.o5(), *a.w, a.fd, 1, None),
    "qtx_greedy_dfault_resume": lambda a: (a.h, 3, 9, 9, *a.o5(), *a.w, a.fd, 1, None, None),
    "qtx_greedy_decode_kvfault": lambda a: (*_DEC(a), *a.o5(), *a.w, a.fd, None, 1, None),
    "qtx_greedy_decode_kvtrials": lambda a: (*_DEC(a), *a.o5(), *a.w, a.trials, None),
    "qtx_greedy_decode_enctrials": lambda a: (*_DEC(a), a.o(), a.o(), a.o(), *a.w, a.faults, None),
    "qtx_score_targets": lambda a: (a.h, a.src, a.m, 3, 9, a.tgt, 9, 1, 2, a.fe, 1, a.o(), a.o(), a.o(), a.o(),
                                    *a.w, None),
}


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("entry", list(REFUSED))
@pytest.mark.parametrize("H", HEADS)
def test_fault_entries_refuse(torch, H, entry, poison):
    """Every entry given a fault: QTX_E_UNSUPPORTED (4), and every output, the workspace and
    their guards keep the poison byte for byte."""
    from types import SimpleNamespace
    from qtx import _lib
    gm, om = model(H)
    src, m, ys, _, _ = greedy_case(("heads", H), om)
    x, em, memory = enc_case(("heads", H), om)
    y, tm, _ = dec_case(("heads", H), om)
    held, bufs = [], []

    def dev(arr):
        held.append(T_(torch, arr))
        return C.c_void_p(held[-1].data_ptr())

    def guard(nbytes):
        bufs.append(guarded(torch, (nbytes,), torch.uint8, poison, name=entry))
        return C.c_void_p(bufs[-1][0].data_ptr())
    f = lambda mod: F.Fault("INPUT", mod, 0, "Q", 0, 5, 3).to_c()
    trials, faults = (_lib.KvTrial * 3)(), (_lib.Fault * 3)()
    trials[0].what, trials[0].step, trials[0].fault, faults[0] = 1, 1, f(1), f(0)
    a = SimpleNamespace(h=gm.handle, src=dev(src), m=dev(m.reshape(3, -1).astype(np.uint8)), x=dev(x),
                        em=dev(em.reshape(3, -1).astype(np.uint8)), y=dev(y), mem=dev(memory),
                        tm=dev(tm[0].astype(np.uint8)), tgt=dev(ys), fe=C.pointer(f(0)), fd=C.pointer(f(1)),
                        trials=trials, faults=faults, o=lambda: guard(1 << 20), o5=lambda: [guard(1 << 20) for _ in range(5)],
                        w=(guard(96 << 20), 96 << 20))
    with pytest.raises(_lib.QtxError) as e:
        _lib.call(entry, *REFUSED[entry](a))
    assert e.value.code == 4, str(e.value)
    torch.cuda.synchronize()
    for payload, chk in bufs:
        chk()
        assert bool((payload == poison).all())


@pytest.mark.parametrize("H", HEADS)
def test_trace_refuses(torch, H):
    from qtx import trace
    gm, om = model(H)
    x, em, _ = enc_case(("heads", H), om)
    with pytest.raises(NotImplementedError):
        trace.trace_encoder(gm, T_(torch, x), u8(torch, em))
