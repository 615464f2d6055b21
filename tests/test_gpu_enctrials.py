"""One independent encoder-side fault trial per sentence (include/qtx_enctrials.h:
qtx_greedy_decode_enctrials; qtx.decode.greedy_decode_enctrials, encfault_campaign) against
tests/enctrials_ref.py, bit for bit: ids, top_ids, top_logp.

Expected values come from the oracle, one sentence at a time, through tests/enctrials_ref.py,
never from the code under test.  Shapes: tests/dfault_cases.py's sentences (S = 14, sentence 1
padded to 9, max_len = 8) over B = 8 and B = 33 rows (M = 462: four row tiles of the table GEMM,
the last ragged, sentence 9 across a tile edge); small models for the FULL tile (M = 128) and the
generic chain.  These are the smallest shapes at which the kernel can still go wrong, not the
workload's.  Faults are written in the coordinates of the decode of their sentence alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enctrials_ref as T  # noqa: E402
from guarded import POISONS, guarded, skewed  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
S, L = T.S, T.L
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4
B8 = len(T.SENT)
bits = T.bits

# Every pointer-taking function of include/qtx_enctrials.h, beside the test ("module::test") that
# runs it with every device pointer — and the workspace — at 16 (mod 256), or the reason it is
# exempt (tests/test_enctrials_abi.py checks the table against the header).
COVERED = {"qtx_greedy_decode_enctrials": "test_gpu_enctrials::test_minimum_alignment",
           "qtx_linear_rows_faults": "test_gpu_rows_faults::test_minimum_alignment"}
EXEMPT = {"qtx_greedy_enctrials_workspace_size": "query on the model handle"}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def decode(model, src, m, faults, max_len=L):
    from qtx.decode import greedy_decode_enctrials
    return greedy_decode_enctrials(model, src, m, max_len, 0, faults)


def same(got, want):
    ys, sc = got
    np.testing.assert_array_equal(ys, want[0])
    assert sc.top_ids.dtype == np.int64 and sc.top_logp.dtype == np.float32
    np.testing.assert_array_equal(sc.top_ids, want[1])
    np.testing.assert_array_equal(bits(sc.top_logp), bits(want[2]))


def check(model, om, src, m, faults, max_len=L):
    exp = T.expect_rows(om, src, m, max_len, faults)
    same(decode(model, src, m, faults, max_len), exp)
    return exp


# =====================================================================================
# 1 / 2. B = 8 and B = 33 against the reference
# =====================================================================================
@pytest.mark.parametrize("name", ["A", "B"])
def test_b8_matches_reference(torch, gpu_model, oracle_model, name):
    src, m = T.batch()
    faults, applied = T.cases()[name]
    exp = check(gpu_model, oracle_model, src, m, faults)
    assert T.changed_rows(oracle_model, src, m, exp) == applied


# six memoised (sentence, fault) pairs: rows of the two tables; row 9 (token rows 126 .. 139,
# across the first tile edge of the table GEMM) gets pair 3, the linear WEIGHT on K
PAIRS33 = (("A", 1), ("A", 2), ("A", 4), ("A", 0), ("B", 1), ("B", 2))


def test_b33_cycles_six_pairs(torch, gpu_model, oracle_model):
    cs = T.cases()
    sent = [T.SENT[PAIRS33[r % 6][1]] for r in range(33)]
    faults = [cs[PAIRS33[r % 6][0]][0][PAIRS33[r % 6][1]] for r in range(33)]
    assert faults[9].kind == "WEIGHT" and faults[9].linear == "K" and 9 * S < 128 < 10 * S
    src, m = T.batch(sent)
    check(gpu_model, oracle_model, src, m, faults)


# =====================================================================================
# 3 / 4 / 5. the FULL tile instance, the generic chain, the forced generic chain
# =====================================================================================
def small_faults(S_):
    from qtx.fault import Fault as F
    return [F("INPUT", 0, 1, "V", row=3, col=50, bit=7),
            F("WEIGHT", 0, 0, "FFN1", row=7, col=100, bit=7),
            F("OUTPUT", 0, 1, "FFN2", row=2, col=100, value=3.0e4),
            None,
            F("WEIGHT", 1, 1, "CK", row=40, col=200, bit=7),
            F("RANDOM", 0, 0, "QK", row=1, col=3 * S_ + 2, value=1.0e4),
            F("INPUT16", 0, 0, "O", row=2, col=40, bit=7, win_start=32, win_len=16),
            F("WEIGHT", 0, 1, "PV", row=2, col=2 * 64 + 7, bit=7)]


def test_full_tiles(torch):
    """M = B * S = 128: every row tile is full, the FULL instances of the table GEMM."""
    from model_cfgs import small_src, small_state
    from qtx.model import QtxModel
    cfg, sd, om = small_state(512, 8, 97)
    src, m = small_src(8, 16, 31, full=(0,))
    faults = small_faults(16)
    exp = check(QtxModel(sd, cfg), om, src, m, faults, max_len=6)
    assert len(T.changed_rows(om, src, m, exp, 6)) >= 4 and np.isfinite(exp[2]).all()


def test_generic_chain(torch):
    """d_ff = 768 (no multiple of 512): self_attn_block / ffn_block with the row-fault GEMM."""
    from model_cfgs import small_src, small_state
    from qtx.model import QtxModel
    cfg, sd, om = small_state(768, 8, 97)
    src, m = small_src(3, 9, 17, full=(0,))
    fs = small_faults(9)
    for faults in ([fs[0], fs[1], fs[4]], [fs[2], fs[5], fs[7]]):
        exp = check(QtxModel(sd, cfg), om, src, m, faults, max_len=6)
        assert T.changed_rows(om, src, m, exp, 6) and np.isfinite(exp[2]).all()


def test_forced_generic_chain(torch, gpu_model, oracle_model, knob_env):
    knob_env("QTX_NO_ROWGEMM", 1)
    src, m = T.batch()
    for faults, _ in T.cases().values():
        check(gpu_model, oracle_model, src, m, faults)


# =====================================================================================
# 6. the decode's path selection
# =====================================================================================
@pytest.mark.parametrize("env,name", [({}, "A"), ({"QTX_NO_GRAPH": 1}, "B"), ({"QTX_UNFUSED": 1}, "A"),
                                      ({"QTX_DECODE_GROUPS": 2}, "B")],
                         ids=["default", "no_graph", "unfused", "groups2"])
def test_paths(torch, gpu_model, oracle_model, knob_env, env, name):
    for k, v in env.items():
        knob_env(k, v)
    src, m = T.batch()
    check(gpu_model, oracle_model, src, m, T.cases()[name][0])


# =====================================================================================
# 7 / 8 / 9. the library's own stand-alone calls, isolation, the campaign helper
# =====================================================================================
def test_rows_equal_the_standalone_call(torch, gpu_model):
    from qtx.decode import greedy_decode_fault, greedy_decode_kvfault
    src, m = T.batch()
    cs = T.cases()
    for name, rows in (("A", (0, 2, 4)), ("B", (2,))):
        faults = cs[name][0]
        ys, sc = decode(gpu_model, src, m, faults)
        for b in rows:
            f = faults[b]
            if f.module == 0:
                y1, s1 = greedy_decode_fault(gpu_model, src[b:b + 1], m[b:b + 1], L, 0, fault=f,
                                             return_scores=True)
            else:
                y1, s1 = greedy_decode_kvfault(gpu_model, src[b:b + 1], m[b:b + 1], L, 0, fault=f,
                                               step=0, return_scores=True)
            np.testing.assert_array_equal(ys[b], np.asarray(y1)[0])
            np.testing.assert_array_equal(sc.top_ids[b], s1.top_ids[0])
            np.testing.assert_array_equal(bits(sc.top_logp[b]), bits(s1.top_logp[0]))


def test_isolation(torch, gpu_model, oracle_model):
    """A token-changing trial on row 0 alone: every other row is the golden scored decode."""
    from qtx.decode import greedy_decode
    src, m = T.batch()
    faults = [T.cases()["B"][0][0]] + [None] * (B8 - 1)
    exp = check(gpu_model, oracle_model, src, m, faults)
    gold = T.expect_rows(oracle_model, src, m, L, [None] * B8)
    assert not np.array_equal(exp[0][0], gold[0][0])
    ys, sc = decode(gpu_model, src, m, faults)
    gy, gs = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    np.testing.assert_array_equal(ys[1:], gy[1:])
    np.testing.assert_array_equal(sc.top_ids[1:], gs.top_ids[1:])
    np.testing.assert_array_equal(bits(sc.top_logp[1:]), bits(gs.top_logp[1:]))
    assert not np.array_equal(ys[0], gy[0])
    # a table of all NONE is the golden scored decode
    ys, sc = decode(gpu_model, src, m, [None] * B8)
    np.testing.assert_array_equal(ys, gy)
    np.testing.assert_array_equal(bits(sc.top_logp), bits(gs.top_logp))


def test_campaign_helper(torch, gpu_model, oracle_model):
    """Five trials on sentence 1 in batches of 4 (the second batch padded): the caller's order."""
    from qtx.decode import encfault_campaign
    import dfault_cases as D
    src, m = D.make_src()
    a, b = T.cases()["A"][0], T.cases()["B"][0]
    faults = [a[1], a[4], b[1], None, b[4]]
    out = encfault_campaign(gpu_model, src[1], m[1], L, faults, batch=4)
    assert len(out) == 5
    for (ys, sc), f in zip(out, faults):
        want = T.expect_row(oracle_model, src[1:2], m[1:2], L, f)
        np.testing.assert_array_equal(ys, want[0])
        np.testing.assert_array_equal(sc.top_ids, want[1])
        np.testing.assert_array_equal(bits(sc.top_logp), bits(want[2]))
    assert encfault_campaign(gpu_model, src[1], m[1], L, [], batch=4) == []


# =====================================================================================
# 10 / 11 / 12. extents, refusals, minimum alignment
# =====================================================================================
def c_faults(faults):
    from qtx import _lib
    arr = (_lib.Fault * len(faults))()
    for b, f in enumerate(faults):
        if f is not None:
            arr[b] = f.to_c()
    return arr


def _outs(torch, poison, B=B8, skew=0):
    spec = (((B, L), torch.int64, "ids"), ((B, L - 1, 2), torch.int64, "top_ids"),
            ((B, L - 1, 2), torch.float32, "top_logp"))
    pairs = [guarded(torch, shp, dt, poison, name=n, skew=skew) for shp, dt, n in spec]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _same_outs(outs, exp):
    np.testing.assert_array_equal(outs[0].cpu().numpy(), exp[0])
    np.testing.assert_array_equal(outs[1].cpu().numpy(), exp[1])
    np.testing.assert_array_equal(bits(outs[2].cpu().numpy()), bits(exp[2]))


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
def test_extents(torch, gpu_model, oracle_model, poison):
    """Exactly ids, top_ids, top_logp are written, each in full; the workspace is not overrun;
    need - 1 bytes: QTX_E_WORKSPACE with everything still poisoned."""
    from qtx import _lib
    L_ = _lib.lib()
    src, m = T.batch()
    faults = T.cases()["A"][0]
    exp = T.expect_rows(oracle_model, src, m, L, faults)
    srcd = torch.from_numpy(src).cuda()
    md = torch.from_numpy(m.reshape(B8, S).astype(np.uint8)).cuda()
    need = L_.qtx_greedy_enctrials_workspace_size(gpu_model.handle, B8, S, L)
    assert need > L_.qtx_greedy_scored_workspace_size(gpu_model.handle, B8, S, L)
    outs, checks = _outs(torch, poison)
    ws, cws = guarded(torch, (need,), torch.uint8, poison, name="workspace")
    head = (gpu_model.handle, P(srcd), P(md), B8, S, L, 0)
    arr = c_faults(faults)
    assert L_.qtx_greedy_decode_enctrials(*head, *[P(t) for t in outs], P(ws), need - 1, arr,
                                          S0) == E_WORKSPACE
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t.view(torch.uint8) == poison).all())
    _lib.call("qtx_greedy_decode_enctrials", *head, *[P(t) for t in outs], P(ws), need, arr, S0)
    gpu_model.check()
    for c in checks + [cws]:
        c()
    _same_outs(outs, exp)


def test_refusals(torch, gpu_model):
    """Each refusal returns its status before anything is launched — the outputs and the
    workspace keep their poison — and names the row."""
    from qtx import _lib
    from qtx.fault import Fault as F
    L_ = _lib.lib()
    src, m = T.batch()
    srcd = torch.from_numpy(src).cuda()
    md = torch.from_numpy(m.reshape(B8, S).astype(np.uint8)).cuda()
    need = L_.qtx_greedy_enctrials_workspace_size(gpu_model.handle, B8, S, L)
    outs, checks = _outs(torch, 0x5A)
    ws, cws = guarded(torch, (need,), torch.uint8, 0x5A, name="workspace")

    def raw(arr, handle=None, nbytes=need):
        rc = L_.qtx_greedy_decode_enctrials(handle or gpu_model.handle, P(srcd), P(md), B8, S, L, 0,
                                            *[P(t) for t in outs], P(ws), nbytes, arr, S0)
        torch.cuda.synchronize()
        if rc != OK:
            for t in outs + [ws]:
                assert bool((t.view(torch.uint8) == 0x5A).all())
            for c in checks + [cws]:
                c()
        return rc

    def call(fault, row=5, **kw):
        faults = [None] * B8
        faults[row] = fault
        rc = raw(c_faults(faults), **kw)
        if rc not in (OK, E_WORKSPACE):
            assert f"row {row}" in L_.qtx_last_error().decode()
        return rc

    assert raw(None) == E_INVALID                                               # table NULL
    assert call(F("INPUT", 1, 2, "Q", row=0, col=0, bit=7)) == E_UNSUPPORTED    # kvtrials' trial
    assert call(F("INPUT", 0, 2, "CQ", row=0, col=0, bit=7)) == E_INVALID
    assert call(F("INPUT", 0, 2, "FFN1", row=S, col=100, bit=6)) == E_INVALID
    assert call(F("OUTPUT", 0, 2, "K", row=0, col=512, value=1.0)) == E_INVALID
    assert call(F("WEIGHT16", 0, 3, "FFN1", row=7, col=100, bit=7, win_start=S - 3, win_len=4)) == E_INVALID
    assert call(F("WEIGHT", 0, 0, "QK", row=S, col=5, bit=7)) == E_INVALID
    assert call(F("WEIGHT", 0, 6, "K", row=40, col=200, bit=7)) == E_INVALID
    assert call(F("INPUT", 0, 1, "V", row=3, col=50, bit=8)) == E_INVALID
    assert call(F("INPUT", 1, 1, "CV", row=S, col=17, bit=7)) == E_INVALID
    assert call(F("INPUT", 0, 1, "V", row=3, col=50, bit=7), nbytes=need - 1) == E_WORKSPACE
    # a 4-bit model
    from model_cfgs import small_state
    from qtx.model import QtxModel
    cfg, sd, _ = small_state(512, 4, 97)
    m4 = QtxModel(sd, cfg)
    assert L_.qtx_greedy_enctrials_workspace_size(m4.handle, B8, S, L) <= need
    srcd.clamp_(max=63)                                                         # its 64-word vocabulary
    assert call(F("INPUT", 0, 1, "V", row=3, col=50, bit=7), handle=m4.handle) == E_UNSUPPORTED
    # the boundaries are accepted
    srcd.copy_(torch.from_numpy(src).cuda())
    assert call(F("INPUT", 0, 2, "FFN1", row=S - 1, col=511, bit=7)) == OK
    assert call(F("WEIGHT16", 0, 3, "FFN1", row=2047, col=511, bit=7, win_start=S - 4, win_len=4)) == OK
    assert call(F("WEIGHT", 0, 0, "QK", row=S - 1, col=511, bit=7), row=7) == OK
    assert call(F("INPUT", 1, 5, "CK", row=S - 1, col=511, bit=7), row=0) == OK


def test_minimum_alignment(torch, gpu_model, oracle_model):
    """One call with every device pointer of the call and the workspace at 16 (mod 256)."""
    from qtx import _lib
    L_ = _lib.lib()
    src, m = T.batch()
    faults = T.cases()["B"][0]
    exp = T.expect_rows(oracle_model, src, m, L, faults)
    srcd = skewed(torch, src, 16)
    md = skewed(torch, m.reshape(B8, S).astype(np.uint8), 16)
    need = L_.qtx_greedy_enctrials_workspace_size(gpu_model.handle, B8, S, L)
    outs, checks = _outs(torch, POISONS[0], skew=16)
    ws, cws = guarded(torch, (need,), torch.uint8, POISONS[0], name="workspace", skew=16)
    for t in [srcd, md, ws] + outs:
        assert t.data_ptr() % 256 == 16
    _lib.call("qtx_greedy_decode_enctrials", gpu_model.handle, P(srcd), P(md), B8, S, L, 0,
              *[P(t) for t in outs], P(ws), need, c_faults(faults), S0)
    gpu_model.check()
    for c in checks + [cws]:
        c()
    _same_outs(outs, exp)
