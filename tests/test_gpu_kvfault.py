"""Faults of the KV-cached decode itself (include/qtx.h: qtx_greedy_decode_kvfault;
qtx.decode.greedy_decode_kvfault) against tests/kvfault_ref.py, bit for bit: ids, top_ids,
top_logp and the record, in the scored and the plain form.

Expected values come from the oracle through tests/kvfault_ref.py, never from the code under
test.  Shapes: tests/dfault_cases.py (B = 3, S = 14 with sentence 1 padded to 9, max_len = 8).
"""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import kvfault_cases as K  # noqa: E402
import kvfault_ref as R  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
B, S, L = D.B, D.S, D.L
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4
CASES = K.cases()
MAIN = ("main", None, L)      # (tag, (src, mask) or None, max_len)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def expect(om, fault, upset, step, inp=MAIN):
    tag, src_m, max_len = inp
    src, m = src_m if src_m is not None else D.make_src()
    return R.trial(om, src, m, max_len, tag, fault, upset, step)


def decode(model, fault, upset, step, scores, inp=MAIN):
    from qtx.decode import greedy_decode_kvfault
    _, src_m, max_len = inp
    src, m = src_m if src_m is not None else D.make_src()
    return greedy_decode_kvfault(model, src, m, max_len, 0, fault=fault, upset=upset, step=step,
                                 return_scores=scores)


def check(model, om, fault, upset, step, inp=MAIN):
    """Scored and plain form against the reference; returns the expectation."""
    exp = expect(om, fault, upset, step, inp)
    ys, sc = decode(model, fault, upset, step, True, inp)
    np.testing.assert_array_equal(ys, exp[0])
    assert sc.top_ids.dtype == np.int64 and sc.top_logp.dtype == np.float32
    np.testing.assert_array_equal(sc.top_ids, exp[1])
    np.testing.assert_array_equal(bits(sc.top_logp), bits(exp[2]))
    r = sc.fault_step
    if exp[3] is None:
        assert r is None
    else:
        assert r is not None and r.step == step
        np.testing.assert_array_equal(r.golden_ids, exp[3][0])
        np.testing.assert_array_equal(bits(r.golden_logp), bits(exp[3][1]))
        np.testing.assert_array_equal(r.faulty_ids, exp[3][2])
        np.testing.assert_array_equal(bits(r.faulty_logp), bits(exp[3][3]))
    # plain form: the oracle's ids are its own first-index argmax (asserted in kvfault_ref._run)
    np.testing.assert_array_equal(decode(model, fault, upset, step, False, inp), exp[0])
    return exp


# =====================================================================================
# 1. every case, scored and plain
# =====================================================================================
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_matches_reference(torch, gpu_model, oracle_model, name):
    check(gpu_model, oracle_model, *CASES[name])


# =====================================================================================
# 2. path selection
# =====================================================================================
# a token-changing V-projection fault (the row k_dec_attn / the row quantizer caches), an
# attention fault on a grouped value, a token-changing self-V upset and a cross-V upset
PATH_CASES = ("in_v_l2_s2", "w_pv_s5_j5", "up_sv_j3", "up_cv_last")


@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_GRAPH_STEPS": 3}, {"QTX_UNFUSED": 1},
                                 {"QTX_DECODE_GROUPS": 2}, {"QTX_DECODE_GROUPS": 2, "QTX_NO_GRAPH": 1}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()) or "default")
def test_paths(torch, gpu_model, oracle_model, knob_env, env):
    """Eager fused steps, graphs of 3 steps, the unfused step (row-major values) and two
    sub-batch groups (the golden ranges on group views, the faulty step on the whole batch) give
    the reference's results; the cross-V upset changes what the step reads on every path."""
    for k, v in env.items():
        knob_env(k, v)
    src, m = D.make_src()
    for name in PATH_CASES:
        exp = check(gpu_model, oracle_model, *CASES[name])
        if name in ("in_v_l2_s2", "up_sv_j3"):
            assert R.effect(oracle_model, src, m, L, "main", exp) == "tokens"
        else:
            assert R.effect(oracle_model, src, m, L, "main", exp) != "none"


@pytest.mark.parametrize("env", [{}, {"QTX_UNFUSED": 1}, {"QTX_NO_GRAPH": 1}, {"QTX_DECODE_GROUPS": 2}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()) or "default")
def test_plain_form_with_record(torch, gpu_model, oracle_model, knob_env, env):
    """top_ids / top_logp NULL, rec_ids / rec_logp given: the record comes from the step's
    logits (the unfused step's generator under QTX_UNFUSED), for a step fault, a memory V
    projection fault and an upset."""
    from qtx import _lib
    for k, v in env.items():
        knob_env(k, v)
    L_ = _lib.lib()
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_kvfault_workspace_size(gpu_model.handle, B, S, L)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for name in ("in_v_l2_s2", "cv_s0", "up_sv_j3"):
        f, u, step = CASES[name]
        exp = expect(oracle_model, f, u, step)
        ids = torch.empty((B, L), dtype=torch.int64, device="cuda")
        ri = torch.empty((B, 2, 2), dtype=torch.int64, device="cuda")
        rl = torch.empty((B, 2, 2), dtype=torch.float32, device="cuda")
        _lib.call("qtx_greedy_decode_kvfault", gpu_model.handle, P(srcd), P(md), B, S, L, 0, P(ids),
                  S0, S0, P(ri), P(rl), P(ws), need,
                  C.byref(f.to_c()) if f is not None else None,
                  C.byref(u.to_c()) if u is not None else None, step, S0)
        gpu_model.check()
        np.testing.assert_array_equal(ids.cpu().numpy(), exp[0])
        np.testing.assert_array_equal(ri.cpu().numpy(), np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(bits(rl.cpu().numpy()),
                                      bits(np.stack([exp[3][1], exp[3][3]], 1)))


def test_long_source_takes_the_unfused_step(torch, gpu_model, oracle_model):
    """S = 132 (above the fused step's 128 keys), max_len = 6."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    inp = ("long", D.make_src(seed=77, b=2, s=132, lens=(132, 70)), 6)
    trials = [(F("OUTPUT", 1, 0, "FFN2", row=0, col=100, value=3.0e4), None, 1),
              (F("INPUT", 1, 2, "V", row=1, col=50, bit=7), None, 2),
              (None, U("cross_v", 0, row=0 * 132 + 131, col=5, bit=7), 1),
              (None, U("self_v", 1, row=1 * 6 + 1, col=70, bit=7), 3)]
    effects = [R.effect(oracle_model, inp[1][0], inp[1][1], 6, "long",
                        check(gpu_model, oracle_model, f, u, s, inp)) for f, u, s in trials]
    assert effects[0] == "tokens" and "none" not in effects


def test_upset_on_a_4bit_model(torch):
    from model_cfgs import small_src, small_state
    from qtx.fault import CacheUpset as U
    from qtx.model import QtxModel
    cfg, sd, om = small_state(512, 4, 97)
    model = QtxModel(sd, cfg)
    inp = ("w4", small_src(3, 9, 17, full=(0,)), L)
    for u, s in ((U("self_v", 1, row=1 * L + 1, col=70, bit=7), 3),
                 (U("cross_k", 0, row=0 * 9 + 3, col=5, bit=7), 1)):
        exp = check(model, om, None, u, s, inp)
        assert R.effect(om, inp[1][0], inp[1][1], L, "w4", exp) != "none"


# =====================================================================================
# 3. identities through the library
# =====================================================================================
@pytest.mark.parametrize("cache", ["self_k", "self_v", "cross_k", "cross_v"])
def test_last_step_upset_equals_transient_weight_fault(torch, gpu_model, oracle_model, cache):
    pairs, i = K.identity_pairs()
    u, f = pairs[cache]
    a = decode(gpu_model, None, u, i, True)
    b = decode(gpu_model, f, None, i, True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].top_ids, b[1].top_ids)
    np.testing.assert_array_equal(bits(a[1].top_logp), bits(b[1].top_logp))
    np.testing.assert_array_equal(bits(a[1].fault_step.faulty_logp), bits(b[1].fault_step.faulty_logp))
    exp = check(gpu_model, oracle_model, None, u, i)
    assert R.effect(oracle_model, *D.make_src(), L, "main", exp) != "none"


@pytest.mark.parametrize("name", ["out_ffn2_l5_s2", "in_co_l5_s3"])
def test_behind_the_kv_projections_equals_the_campaign_decode(torch, gpu_model, name):
    """Last layer, behind the K/V projections: the caches stay golden, so the cached-step
    fault and the campaign's full-prefix fault (row moved to the last prefix position) agree."""
    from qtx.decode import greedy_decode_fault
    f, _, i = CASES[name]
    src, m = D.make_src()
    fc = dataclasses.replace(f, row=f.row * (i + 1) + i)
    a = decode(gpu_model, f, None, i, True)
    b = greedy_decode_fault(gpu_model, src, m, L, 0, fault=fc, target_inference_number=i + 1,
                            return_scores=True, kv_cache=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].top_ids, b[1].top_ids)
    np.testing.assert_array_equal(bits(a[1].top_logp), bits(b[1].top_logp))
    for k in ("golden_ids", "faulty_ids"):
        np.testing.assert_array_equal(getattr(a[1].fault_step, k), getattr(b[1].fault_step, k))


# =====================================================================================
# 4. extents and refusals
# =====================================================================================
def _dev_inputs(torch):
    src, m = D.make_src()
    return (torch.from_numpy(src).cuda(),
            torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda())


def _outs(torch, poison):
    spec = (((B, L), torch.int64, "ids"), ((B, L - 1, 2), torch.int64, "top_ids"),
            ((B, L - 1, 2), torch.float32, "top_logp"), ((B, 2, 2), torch.int64, "rec_ids"),
            ((B, 2, 2), torch.float32, "rec_logp"))
    pairs = [guarded(torch, shp, dt, poison, name=n) for shp, dt, n in spec]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
@pytest.mark.parametrize("name", ["in_v_l2_s2", "up_sv_j3", "never"])
def test_extents(torch, gpu_model, oracle_model, name, poison):
    """Exactly ids, top_ids, top_logp, rec_ids, rec_logp are written, each in full; a trial
    that is never applied leaves the record untouched; the workspace is not overrun."""
    from qtx import _lib
    L_ = _lib.lib()
    f, u, step = CASES[name]
    exp = expect(oracle_model, f, u, step)
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_kvfault_workspace_size(gpu_model.handle, B, S, L)
    assert need > L_.qtx_greedy_scored_workspace_size(gpu_model.handle, B, S, L)
    outs, checks = _outs(torch, poison)
    ws, cws = guarded(torch, (need,), torch.uint8, poison, name="workspace")
    fc = C.byref(f.to_c()) if f is not None else None
    uc = C.byref(u.to_c()) if u is not None else None
    head = (gpu_model.handle, P(srcd), P(md), B, S, L, 0)
    assert L_.qtx_greedy_decode_kvfault(*head, *[P(t) for t in outs], P(ws), need - 1, fc, uc,
                                        step, S0) == E_WORKSPACE
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t.view(torch.uint8) == poison).all())
    _lib.call("qtx_greedy_decode_kvfault", *head, *[P(t) for t in outs], P(ws), need, fc, uc, step, S0)
    gpu_model.check()
    for c in checks + [cws]:
        c()
    ids, ti, tl, ri, rl = outs
    np.testing.assert_array_equal(ids.cpu().numpy(), exp[0])
    np.testing.assert_array_equal(ti.cpu().numpy(), exp[1])
    np.testing.assert_array_equal(bits(tl.cpu().numpy()), bits(exp[2]))
    if exp[3] is None:
        assert bool((ri.view(torch.uint8) == poison).all()) and bool((rl.view(torch.uint8) == poison).all())
    else:
        np.testing.assert_array_equal(ri.cpu().numpy(), np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(bits(rl.cpu().numpy()), bits(np.stack([exp[3][1], exp[3][3]], 1)))
    # the plain form writes ids alone; with a record asked for, that too
    outs2, checks2 = _outs(torch, poison)
    _lib.call("qtx_greedy_decode_kvfault", *head, P(outs2[0]), S0, S0, P(outs2[3]), P(outs2[4]),
              P(ws), need, fc, uc, step, S0)
    gpu_model.check()
    for c in checks2 + [cws]:
        c()
    np.testing.assert_array_equal(outs2[0].cpu().numpy(), exp[0])
    for t in outs2[1:3]:
        assert bool((t.view(torch.uint8) == poison).all())
    if exp[3] is not None:
        np.testing.assert_array_equal(outs2[3].cpu().numpy(), np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(bits(outs2[4].cpu().numpy()),
                                      bits(np.stack([exp[3][1], exp[3][3]], 1)))
    else:
        assert bool((outs2[3].view(torch.uint8) == poison).all())


def test_refusals(torch, gpu_model, state_dict):
    """Each refusal returns its status before anything is launched: the outputs and the
    workspace keep their poison."""
    from qtx import _lib
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig
    L_ = _lib.lib()
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_kvfault_workspace_size(gpu_model.handle, B, S, L)
    outs, checks = _outs(torch, 0x5A)
    ws, cws = guarded(torch, (need,), torch.uint8, 0x5A, name="workspace")

    def call(model, f, u, step, nbytes=need):
        rc = L_.qtx_greedy_decode_kvfault(
            model.handle, P(srcd), P(md), B, S, L, 0, *[P(t) for t in outs], P(ws), nbytes,
            C.byref(f.to_c()) if f is not None else None,
            C.byref(u.to_c()) if u is not None else None, step, S0)
        torch.cuda.synchronize()
        if rc != OK:
            for t in outs + [ws]:
                assert bool((t.view(torch.uint8) == 0x5A).all())
            for c in checks + [cws]:
                c()
        return rc

    good_f = F("INPUT", 1, 2, "FFN1", row=0, col=100, bit=6)
    good_u = U("self_k", 0, row=0 * L + 1, col=33, bit=7)
    assert call(gpu_model, good_f, good_u, 3) == E_INVALID            # both
    assert call(gpu_model, None, None, 3) == E_INVALID                # neither
    assert call(gpu_model, F("INPUT", 0, 2, "FFN1", row=0, col=100, bit=6), None, 3) == E_INVALID
    assert call(gpu_model, F("NONE", 1, 2, "FFN1"), None, 3) == E_INVALID
    assert call(gpu_model, good_f, None, -1) == E_INVALID
    # coordinates of the step's own shapes: rows [B], self keys step + 1
    assert call(gpu_model, F("INPUT", 1, 2, "FFN1", row=B, col=100, bit=6), None, 3) == E_INVALID
    assert call(gpu_model, F("OUTPUT", 1, 2, "K", row=0, col=512, value=1.0), None, 3) == E_INVALID
    assert call(gpu_model, F("WEIGHT", 1, 0, "QK", row=B * 4, col=5, bit=7), None, 3) == E_INVALID
    assert call(gpu_model, F("INPUT16", 1, 0, "QK", row=0, col=5, bit=7, win_start=0, win_len=5),
                None, 3) == E_INVALID
    assert call(gpu_model, F("INPUT", 1, 0, "PV", row=0, col=7 * 4 + 4, bit=7), None, 3) == E_INVALID
    assert call(gpu_model, F("INPUT", 1, 0, "CQK", row=B, col=0, bit=7), None, 3) == E_INVALID
    assert call(gpu_model, F("WEIGHT", 1, 1, "CK", row=40, col=200, bit=7), None, 1) == E_INVALID
    assert call(gpu_model, F("WEIGHT", 1, 6, "K", row=40, col=200, bit=7), None, 1) == E_INVALID
    # upsets: j >= i, a scale's exponent bit, col / row / cache / layer out of range
    assert call(gpu_model, None, U("self_k", 0, row=0 * L + 3, col=33, bit=7), 3) == E_INVALID
    assert call(gpu_model, None, U("self_v", 0, row=0, col=33, bit=7), 0) == E_INVALID
    for bit in (23, 30, 32, -1):
        assert call(gpu_model, None, U("self_k", 0, row=1, bit=bit, field="scale"), 3) == E_INVALID
    assert call(gpu_model, None, U("self_k", 0, row=1, col=1, bit=3, field="scale"), 3) == E_INVALID
    assert call(gpu_model, None, U("self_k", 0, row=1, col=512, bit=7), 3) == E_INVALID
    assert call(gpu_model, None, U("self_k", 0, row=1, col=33, bit=8), 3) == E_INVALID
    assert call(gpu_model, None, U("cross_v", 0, row=B * S, col=33, bit=7), 3) == E_INVALID
    assert call(gpu_model, None, U("self_k", 0, row=B * L + 1, col=33, bit=7), 3) == E_INVALID
    assert call(gpu_model, None, U("cross_k", 6, row=0, col=33, bit=7), 3) == E_INVALID
    bad = good_u.to_c()
    bad.cache = 4
    assert L_.qtx_greedy_decode_kvfault(gpu_model.handle, P(srcd), P(md), B, S, L, 0,
                                        *[P(t) for t in outs], P(ws), need, None, C.byref(bad), 3,
                                        S0) == E_INVALID
    assert call(gpu_model, good_f, None, 3, need - 1) == E_WORKSPACE
    assert call(gpu_model, None, good_u, 3, need - 1) == E_WORKSPACE
    m4 = QtxModel(state_dict, ModelConfig(weight_bits=4))
    assert call(m4, good_f, None, 3) == E_UNSUPPORTED
    del m4
    # the boundaries are accepted
    assert call(gpu_model, F("WEIGHT", 1, 0, "QK", row=0 * 4 + 3, col=5, bit=7), None, 3) == OK
    assert call(gpu_model, None, U("self_k", 0, row=0 * L + 2, bit=22, field="scale"), 3) == OK
    gpu_model.check()


# =====================================================================================
# 5. neighbours undisturbed
# =====================================================================================
def test_neighbours_undisturbed(torch, gpu_model):
    from qtx import decode_fault_sweep
    from qtx.decode import greedy_decode
    src, m = D.make_src()
    t = D.trials()
    trials = [t[n] for n in ("output_ffn2_t2", "input_bit0_t2", "last_step")]

    def neighbours():
        ys, sc = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
        res, _ = decode_fault_sweep(gpu_model, src, m, L, 0, trials)
        flat = [ys, sc.top_ids, bits(sc.top_logp), greedy_decode(gpu_model, src, m, L, 0)]
        for y, s in res:
            flat += [y, s.top_ids, bits(s.top_logp)]
        return flat

    before = neighbours()
    for name in ("in_v_l2_s2", "rand_qk_s4", "up_cv_last", "ck_s0"):
        decode(gpu_model, *CASES[name], True)
    for a, b in zip(neighbours(), before):
        np.testing.assert_array_equal(a, b)
