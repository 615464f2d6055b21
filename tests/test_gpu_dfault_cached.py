"""The KV-cached decode with a decoder fault (include/qtx.h: qtx_greedy_decode_dfault,
qtx_greedy_dfault_resume; qtx.decode greedy_decode_fault(kv_cache=True), decode_fault_sweep)
against the oracle, bit for bit.

Expected values come from tests/dfault_cases.py: the campaign loop on the oracle
(oracle_model.decode(..., fault=) + generator per step, ids checked against
oracle_model.greedy_decode(fault=, fault_step=)), never from the code under test.  B = 3,
S = 14 with sentence 1 padded to 9, max_len = 8.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
B, S, L = D.B, D.S, D.L
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def expect(om, name, tag="main", src_m=None, max_len=L):
    f, tin = D.trials()[name]
    src, m = src_m if src_m is not None else D.make_src()
    return D.oracle_trial(om, src, m, max_len, f, tin, tag)


def check_scored(got, exp, tin, max_len=L):
    ys, sc = got
    np.testing.assert_array_equal(ys, exp[0])
    assert sc.top_ids.dtype == np.int64 and sc.top_logp.dtype == np.float32
    np.testing.assert_array_equal(sc.top_ids, exp[1])
    np.testing.assert_array_equal(sc.top_logp, exp[2])
    r = sc.fault_step
    if exp[3] is None:
        assert r is None
        return
    assert r is not None and r.step == tin - 1
    np.testing.assert_array_equal(r.golden_ids, exp[3][0])
    np.testing.assert_array_equal(r.golden_logp, exp[3][1])
    np.testing.assert_array_equal(r.faulty_ids, exp[3][2])
    np.testing.assert_array_equal(r.faulty_logp, exp[3][3])
    np.testing.assert_array_equal(r.token_changed, exp[3][0][:, 0] != exp[3][2][:, 0])


def cached(model, f, tin, scores, src_m=None, max_len=L):
    from qtx.decode import greedy_decode_fault
    src, m = src_m if src_m is not None else D.make_src()
    return greedy_decode_fault(model, src, m, max_len, 0, fault=f, target_inference_number=tin,
                               return_scores=scores, kv_cache=True)


# =====================================================================================
# 1. single trials, scored and plain
# =====================================================================================
SINGLE = ("input_ffn1", "weight_o", "weight_ffn2", "weight16_cv", "random_qk", "input_pv",
          "output_ffn2", "input_v_pos0", "first_step", "last_step", "never_8", "never_11")


@pytest.fixture(scope="module")
def covered(oracle_model):
    """The single trials cannot pass on masked faults alone, nor on token changers alone:
    asserted on the oracle's results, once."""
    ch = {n: D.changed(expect(oracle_model, n)) for n in SINGLE}
    assert any(ch.values()) and not all(ch[n] for n in SINGLE if not n.startswith("never"))
    assert ch["output_ffn2"] and ch["weight_ffn2"] and not ch["input_ffn1"]
    return ch


@pytest.mark.parametrize("name", SINGLE)
def test_single_trial_matches_oracle(torch, gpu_model, oracle_model, covered, name):
    f, tin = D.trials()[name]
    exp = expect(oracle_model, name)
    check_scored(cached(gpu_model, f, tin, True), exp, tin)
    # plain form: the oracle's ids are its own first-index argmax, the plain rule (asserted
    # equal to its top 1 in dfault_cases._step)
    np.testing.assert_array_equal(cached(gpu_model, f, tin, False), exp[0])


def test_equals_the_full_prefix_loop(torch, gpu_model):
    """kv_cache=True returns what today's loop (kv_cache=False) returns, scored and plain."""
    from qtx.decode import greedy_decode_fault
    src, m = D.make_src()
    for name in ("output_ffn2", "weight16_cv"):
        f, tin = D.trials()[name]
        a = greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, target_inference_number=tin,
                                return_scores=True)
        b = cached(gpu_model, f, tin, True)
        np.testing.assert_array_equal(b[0], a[0])
        np.testing.assert_array_equal(b[1].top_ids, a[1].top_ids)
        np.testing.assert_array_equal(b[1].top_logp, a[1].top_logp)
        for k in ("step", "golden_ids", "golden_logp", "faulty_ids", "faulty_logp"):
            np.testing.assert_array_equal(getattr(b[1].fault_step, k), getattr(a[1].fault_step, k))
        np.testing.assert_array_equal(
            cached(gpu_model, f, tin, False),
            greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, target_inference_number=tin))


# =====================================================================================
# 2. path selection
# =====================================================================================
def _path_trials():
    """A WEIGHT trial (it changes sentence 2's token at step 2: the `covered` fixture) and an
    INPUT trial on sentence 2, each at step 1 and 2."""
    from qtx.fault import Fault
    t = D.trials()
    out = []
    for tin in (2, 3):
        out.append((t["weight_ffn2"][0], tin))
        out.append((Fault("INPUT", 1, 2, "FFN1", row=2 * tin + tin - 1, col=100, bit=6), tin))
    return out


def _run_paths(model):
    res = []
    for f, tin in _path_trials():
        ys, sc = cached(model, f, tin, True)
        r = sc.fault_step
        res.append((ys, sc.top_ids, sc.top_logp, r.golden_ids, r.golden_logp, r.faulty_ids,
                    r.faulty_logp, cached(model, f, tin, False)))
    return res


@pytest.fixture(scope="module")
def paths_default(torch, gpu_model, oracle_model, covered):
    res = _run_paths(gpu_model)
    src, m = D.make_src()
    for (f, tin), r in zip(_path_trials(), res):      # the default itself equals the oracle
        exp = D.oracle_trial(oracle_model, src, m, L, f, tin, "main")
        np.testing.assert_array_equal(r[0], exp[0])
        np.testing.assert_array_equal(r[2], exp[2])
    return res


@pytest.mark.parametrize("env", [{"QTX_NO_GRAPH": 1}, {"QTX_UNFUSED": 1}, {"QTX_GRAPH_STEPS": 3},
                                 {"QTX_DECODE_GROUPS": 2},
                                 {"QTX_DECODE_GROUPS": 2, "QTX_NO_GRAPH": 1}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()))
def test_paths_agree(torch, gpu_model, paths_default, knob_env, env):
    """Eager launches, the unfused step, graphs of 3 steps with the fault at step 1 (inside a
    graph of the plain decode) and step 2 (its last), and sub-batch groups give the default
    path's results."""
    for k, v in env.items():
        knob_env(k, v)
    for got, want in zip(_run_paths(gpu_model), paths_default):
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


# =====================================================================================
# 3. other model configs (the unfused step; a vocabulary above the fused tail's cap)
# =====================================================================================
@pytest.mark.parametrize("key", [(1024, 8, 97), (512, 8, 8200)], ids=["dff1024", "vocab8200"])
def test_configs(torch, key):
    from model_cfgs import small_src, small_state
    from qtx.fault import Fault
    from qtx.model import QtxModel
    cfg, sd, om = small_state(*key)
    model = QtxModel(sd, cfg)
    src_m = small_src(3, 9, 17, full=(0,))
    tin = 3
    f = Fault("OUTPUT", 1, cfg.n_layers - 1, "FFN2", row=1 * tin + tin - 1, col=7, value=3.0e4)
    exp = D.oracle_trial(om, src_m[0], src_m[1], L, f, tin, "cfg%d_%d" % (key[0], key[2]))
    check_scored(cached(model, f, tin, True, src_m), exp, tin)
    np.testing.assert_array_equal(cached(model, f, tin, False, src_m), exp[0])
    f2 = Fault("WEIGHT", 1, 0, "O", row=5, col=9, bit=6)
    exp = D.oracle_trial(om, src_m[0], src_m[1], L, f2, 5, "cfg%d_%d" % (key[0], key[2]))
    check_scored(cached(model, f2, 5, True, src_m), exp, 5)


# =====================================================================================
# 4. extents
# =====================================================================================
def _dev_inputs(torch):
    src, m = D.make_src()
    return (torch.from_numpy(src).cuda(),
            torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda())


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
@pytest.mark.parametrize("name", ["output_ffn2", "never_8"])
def test_extents(torch, gpu_model, oracle_model, name, poison):
    """Exactly ids, top_ids, top_logp, rec_ids, rec_logp are written, each in full (an
    unwritten element keeps the poison, which cannot equal the expectation under both bytes);
    a never-applied fault leaves the record untouched; the workspace is not overrun."""
    from qtx import _lib
    L_ = _lib.lib()
    f, tin = D.trials()[name]
    exp = expect(oracle_model, name)
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_dfault_workspace_size(gpu_model.handle, B, S, L)
    assert need > L_.qtx_greedy_scored_workspace_size(gpu_model.handle, B, S, L)
    ids, c0 = guarded(torch, (B, L), torch.int64, poison, name="ids")
    ti, c1 = guarded(torch, (B, L - 1, 2), torch.int64, poison, name="top_ids")
    tl, c2 = guarded(torch, (B, L - 1, 2), torch.float32, poison, name="top_logp")
    ri, c3 = guarded(torch, (B, 2, 2), torch.int64, poison, name="rec_ids")
    rl, c4 = guarded(torch, (B, 2, 2), torch.float32, poison, name="rec_logp")
    ws, c5 = guarded(torch, (need,), torch.uint8, poison, name="workspace")
    fc = f.to_c()
    args = (gpu_model.handle, P(srcd), P(md), B, S, L, 0, P(ids), P(ti), P(tl), P(ri), P(rl), P(ws))
    assert L_.qtx_greedy_decode_dfault(*args, need - 1, C.byref(fc), tin - 1, S0) == E_WORKSPACE
    torch.cuda.synchronize()
    for t in (ids, ti, tl, ri, rl, ws):
        assert bool((t.view(torch.uint8) == poison).all())
    _lib.call("qtx_greedy_decode_dfault", *args, need, C.byref(fc), tin - 1, S0)
    gpu_model.check()
    for c in (c0, c1, c2, c3, c4, c5):
        c()
    np.testing.assert_array_equal(ids.cpu().numpy(), exp[0])
    np.testing.assert_array_equal(ti.cpu().numpy(), exp[1])
    np.testing.assert_array_equal(tl.cpu().numpy(), exp[2])
    if exp[3] is None:
        assert bool((ri.view(torch.uint8) == poison).all()) and bool((rl.view(torch.uint8) == poison).all())
    else:
        np.testing.assert_array_equal(ri.cpu().numpy(), np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(rl.cpu().numpy(), np.stack([exp[3][1], exp[3][3]], 1))
    # the plain form writes ids alone; with a record asked for, that too
    ids2, d0 = guarded(torch, (B, L), torch.int64, poison, name="ids (plain)")
    ri2, d3 = guarded(torch, (B, 2, 2), torch.int64, poison, name="rec_ids (plain)")
    rl2, d4 = guarded(torch, (B, 2, 2), torch.float32, poison, name="rec_logp (plain)")
    _lib.call("qtx_greedy_decode_dfault", gpu_model.handle, P(srcd), P(md), B, S, L, 0, P(ids2), S0,
              S0, P(ri2), P(rl2), P(ws), need, C.byref(fc), tin - 1, S0)
    gpu_model.check()
    for c in (d0, d3, d4, c5):
        c()
    np.testing.assert_array_equal(ids2.cpu().numpy(), exp[0])
    if exp[3] is not None:
        np.testing.assert_array_equal(ri2.cpu().numpy(), np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(rl2.cpu().numpy(), np.stack([exp[3][1], exp[3][3]], 1))
    else:
        assert bool((ri2.view(torch.uint8) == poison).all())


# =====================================================================================
# 5. refusals
# =====================================================================================
def test_refusals(torch, gpu_model, state_dict):
    """Each refusal returns its status before anything is launched: the outputs keep their
    poison, and a golden scored decode afterwards equals one made before."""
    from qtx import _lib
    from qtx.decode import greedy_decode
    from qtx.fault import Fault
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig
    L_ = _lib.lib()
    src, m = D.make_src()
    before = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_dfault_workspace_size(gpu_model.handle, B, S, L)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ws2 = torch.zeros(need, dtype=torch.uint8, device="cuda")   # fresh: no stamp, no header
    outs = [guarded(torch, shp, dt, 0x5A, name=n)[0] for shp, dt, n in
            (((B, L), torch.int64, "ids"), ((B, L - 1, 2), torch.int64, "top_ids"),
             ((B, L - 1, 2), torch.float32, "top_logp"), ((B, 2, 2), torch.int64, "rec_ids"),
             ((B, 2, 2), torch.float32, "rec_logp"))]
    po = [P(t) for t in outs]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == 0x5A).all()) for t in outs)

    def dfault(model, fault, step, w=ws):
        return L_.qtx_greedy_decode_dfault(model.handle, P(srcd), P(md), B, S, L, 0, *po, P(w), need,
                                           C.byref(fault.to_c()) if fault is not None else None,
                                           step, S0)

    def resume(fault, step, w=ws, shape=(B, S, L)):
        ch = (C.c_int32 * B)()
        return L_.qtx_greedy_dfault_resume(gpu_model.handle, *shape, *po, P(w), need,
                                           C.byref(fault.to_c()), step, ch, S0)

    good = Fault("INPUT", 1, 2, "FFN1", row=0, col=100, bit=6)
    assert dfault(gpu_model, Fault("INPUT", 0, 2, "FFN1", row=0, col=100, bit=6), 2) == E_INVALID
    assert dfault(gpu_model, None, 2) == E_INVALID
    assert dfault(gpu_model, Fault("NONE", 1, 2, "FFN1"), 2) == E_INVALID
    assert dfault(gpu_model, good, -1) == E_INVALID
    T = 3                                        # fault_step 2: rows 0 .. B*T - 1
    assert dfault(gpu_model, Fault("INPUT", 1, 2, "FFN1", row=B * T, col=100, bit=6), T - 1) == E_INVALID
    assert dfault(gpu_model, Fault("INPUT", 1, 2, "FFN1", row=B * T - 1, col=100, bit=6), T - 1) == OK
    gpu_model.check()
    for t in outs:
        t.view(torch.uint8).fill_(0x5A)
    m4 = QtxModel(state_dict, ModelConfig(weight_bits=4))
    assert dfault(m4, good, 2) == E_UNSUPPORTED
    del m4
    # resume: a fresh workspace; other shapes; a step above the golden prefix
    assert resume(good, 1, w=ws2) == E_INVALID
    assert untouched()
    assert dfault(gpu_model, good, 2, w=ws2) == OK      # applied at step 2: n = 2
    gpu_model.check()
    for t in outs:
        t.view(torch.uint8).fill_(0x5A)
    assert resume(good, 1, w=ws2, shape=(B, S, L - 1)) == E_INVALID
    assert resume(good, 1, w=ws2, shape=(B - 1, S, L)) == E_INVALID
    assert resume(good, 4, w=ws2) == E_INVALID
    assert resume(Fault("INPUT", 0, 2, "FFN1", row=0, col=100, bit=6), 1, w=ws2) == E_INVALID
    assert resume(Fault("INPUT", 1, 2, "FFN1", row=B * 2, col=100, bit=6), 1, w=ws2) == E_INVALID
    assert untouched()
    assert resume(good, 2, w=ws2) == OK
    keep = ws2.clone()                           # overwritten by someone else: the stamp is gone
    ws2.zero_()
    assert resume(good, 1, w=ws2) == E_INVALID
    ws2.copy_(keep)
    assert resume(good, 1, w=ws2) == E_INVALID   # (and the header went with it)
    assert dfault(gpu_model, good, 2, w=ws2) == OK
    gpu_model.check()
    # a plain scored decode on that workspace drops its header
    ti = torch.empty((B, L - 1, 2), dtype=torch.int64, device="cuda")
    tl = torch.empty((B, L - 1, 2), dtype=torch.float32, device="cuda")
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")
    _lib.call("qtx_greedy_decode_scored", gpu_model.handle, P(srcd), P(md), B, S, L, 0, P(ids), P(ti),
              P(tl), P(ws2), need, None, S0)
    assert resume(good, 1, w=ws2) == E_INVALID
    after = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1].top_ids, before[1].top_ids)
    np.testing.assert_array_equal(after[1].top_logp, before[1].top_logp)
    np.testing.assert_array_equal(ids.cpu().numpy(), before[0])


# =====================================================================================
# 6. the sweep
# =====================================================================================
def test_sweep(torch, gpu_model, oracle_model):
    """Eight trials (target inference numbers 1, 2, 2, 4, 6, 7 and two never applied), in the
    caller's order, reversed and shuffled: every trial equals the oracle's and the single
    call's result whatever ran before it on the workspace."""
    from qtx import decode_fault_sweep
    from qtx.decode import greedy_decode
    src, m = D.make_src()
    before = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    t = D.trials()
    names = list(D.SWEEP)
    assert sorted(t[n][1] for n in names) == [1, 2, 2, 4, 6, 7, L, L + 3]
    exp = {n: expect(oracle_model, n) for n in names}
    assert not D.changed(exp["input_bit0_t2"])                       # the masked one
    assert D.changed(exp["output_ffn2_t2"]) and D.changed(exp["output_ffn2_late"])
    assert t["output_ffn2_t2"][1] < t["output_ffn2_late"][1]         # the earlier and the later
    orders = [names, names[::-1], random.Random(3).sample(names, len(names))]
    for order in orders:
        res, stats = decode_fault_sweep(gpu_model, src, m, L, 0, [t[n] for n in order])
        assert stats.n_trials == len(order) and len(res) == len(order)
        assert stats.n_skipped >= 1 and stats.n_resumed >= 2 and stats.n_never == 2
        assert stats.n_skipped + stats.n_resumed + stats.n_never == stats.n_trials
        for n, got in zip(order, res):
            check_scored(got, exp[n], t[n][1])
    for n in ("output_ffn2_t2", "input_bit0_t2", "last_step"):       # and the single call's
        one = cached(gpu_model, *t[n], True)
        check_scored(one, exp[n], t[n][1])
    after = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1].top_ids, before[1].top_ids)
    np.testing.assert_array_equal(after[1].top_logp, before[1].top_logp)
