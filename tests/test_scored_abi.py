"""The scored decode's C-ABI and Python surface without a GPU: exported symbols, argument
errors that need no device, the Scores record, the kernel-argument preload of the new tail
kernel, and the pin of csrc/qtx_common.h:qlog against the oracle's float32 log."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import qtx_oracle as O
from qtx import _build, _lib

f32 = np.float32
NEW = ("qtx_greedy_decode_scored", "qtx_greedy_scored_workspace_size", "qtx_generator_top2",
       "qtx_decode_top2_embed")
E_INVALID = 1


def test_new_symbols_exported_and_bound():
    L = ctypes.CDLL(_build.build())
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert name in _lib.header_symbols(), name


def test_scored_workspace_size_without_model_is_zero():
    L = _lib.lib()
    assert L.qtx_greedy_scored_workspace_size(None, 2, 16, 72) == 0
    assert L.qtx_greedy_workspace_size(None, 2, 16, 72) == 0


def test_null_arguments_are_invalid_without_gpu():
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced
    assert L.qtx_greedy_decode_scored(None, one, one, 1, 4, 4, 0, one, one, one, one, 1 << 20,
                                      None, None) == E_INVALID
    assert b"null" in L.qtx_last_error()
    assert L.qtx_generator_top2(None, one, 1, one, one, one, 1 << 20, None) == E_INVALID
    assert L.qtx_decode_top2_embed(None, one, 1, one, 8, one, one, one, one, None) == E_INVALID


def test_scores_margin():
    from qtx.decode import FaultStepRecord, Scores
    lp = np.array([[[-0.25, -1.75], [-0.5, -0.5]], [[-1.0, -3.0], [np.nan, np.nan]]], f32)
    ids = np.array([[[7, 3], [2, 9]], [[1, 0], [0, 1]]], np.int64)
    s = Scores(ids, lp)
    assert s.fault_step is None
    m = s.margin
    assert m.shape == (2, 2) and m.dtype == f32
    np.testing.assert_array_equal(m[0], f32([1.5, 0.0]))
    assert m[1, 0] == f32(2.0) and np.isnan(m[1, 1])
    torch = pytest.importorskip("torch")
    st = Scores(torch.from_numpy(ids), torch.from_numpy(lp))
    np.testing.assert_array_equal(st.margin[0].numpy(), f32([1.5, 0.0]))
    r = FaultStepRecord(2, np.array([[5, 1]]), lp[0, :1], np.array([[1, 5]]), lp[0, 1:])
    assert r.token_changed.tolist() == [True]
    r = FaultStepRecord(2, np.array([[5, 1]]), lp[0, :1], np.array([[5, 2]]), lp[0, 1:])
    assert r.token_changed.tolist() == [False]


def qlog_mirror(x):
    """csrc/qtx_common.h:qlog, operation by operation (fma32: the correctly rounded fma)."""
    H = lambda h: f32(float.fromhex(h))
    x = np.asarray(x, f32)
    m, e = np.frexp(x)                              # m in [0.5, 1)
    m, e = m.astype(f32), e.astype(f32)
    low = m <= H("0x1.6a09e6p-1")
    m = np.where(low, m * f32(2), m).astype(f32)
    e = np.where(low, e - f32(1), e).astype(f32)
    y = (m - f32(1)).astype(f32)
    p = np.full(y.shape, H("0x1.a8579ap-6"), f32)
    for c in ("0x1.860666p-2", "0x1.7ae152p+0", "0x1.0e6c38p+1", "0x1p+0", "0x0p+0"):
        p = O.fma32(p, y, H(c))
    q = np.full(y.shape, H("0x1.8107bep-8"), f32)
    for c in ("0x1.3cb7e6p-3", "0x1.f915c8p-1", "0x1.39fc1ap+1", "0x1.4e6c38p+1", "0x1p+0"):
        q = O.fma32(q, y, H(c))
    return O.fma32(e, H("0x1.62e43p-1"), (p / q).astype(f32))


def test_qlog_is_the_oracles_log():
    """The scored kernels take the log of the log-softmax denominator with qlog so that their
    log-probabilities equal the oracle's bit for bit; the oracle takes it with the host's
    float32 np.log.  This pins the two against each other over a denominator's range
    [1, 8192] and beyond (if the host's log ever changes, this test says so before the GPU
    tests do)."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(1, 8192, 200000), rng.uniform(1, 4, 100000),
                        1 + rng.uniform(0, 1e-3, 50000), rng.uniform(8192, 1e6, 50000),
                        2.0 ** np.arange(0, 20), [1.4142135, 1.4142137, 0.70710677 * 2]]).astype(f32)
    np.testing.assert_array_equal(qlog_mirror(x), np.log(x))
    # and the constants of the mirror are the kernel's
    src = open(os.path.join(_build.CSRC, "qtx_common.h")).read()
    body = src[src.index("float qlog(float x)"):]
    body = body[:body.index("\n}\n")]
    for c in ("0x1.6a09e6p-1f", "0x1.a8579ap-6f", "0x1.860666p-2f", "0x1.7ae152p+0f",
              "0x1.0e6c38p+1f", "0x1.8107bep-8f", "0x1.3cb7e6p-3f", "0x1.f915c8p-1f",
              "0x1.39fc1ap+1f", "0x1.4e6c38p+1f", "0x1.62e43p-1f"):
        assert c in body, c


def test_top2_tail_kernel_preloads_its_arguments(tmp_path):
    """As tests/test_kernarg_preload.py, for k_top2_embed: its leading scalar parameters
    arrive in SGPRs (a non-zero .amdhsa_user_sgpr_kernarg_preload_length)."""
    try:
        hipcc = _build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not installed")
    src = os.path.join(_build.CSRC, "qtx_decode.hip")
    out = tmp_path / "decode.s"
    subprocess.run([hipcc, *_build.compile_flags(src), "--cuda-device-only", "-S", "-o", str(out), src],
                   check=True, capture_output=True, timeout=900)
    lengths, cur = {}, None
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            lengths[cur] = 0
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
        if m and cur:
            lengths[cur] = int(m.group(1))
        if ".end_amdhsa_kernel" in line:
            cur = None
    mine = {k: n for k, n in lengths.items() if "k_top2_embed" in k}
    assert mine, "no k_top2_embed kernel in the code object"
    assert all(n > 0 for n in mine.values()), mine
