"""One independent kvfault trial per sentence (include/qtx.h: qtx_greedy_decode_kvtrials;
qtx.decode.greedy_decode_kvfault_trials, kvfault_campaign) against tests/kvtrials_ref.py, bit for
bit: ids, top_ids, top_logp and the records.

Expected values come from the oracle, one sentence at a time, through tests/kvtrials_ref.py,
never from the code under test.  Shapes: tests/dfault_cases.py's sentences (S = 14, sentence 1
padded to 9, max_len = 8) repeated over B = 8 and B = 33 rows.  Trials are written in the
coordinates of the decode of their sentence alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import kvtrials_ref as T  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
S, L = D.S, D.L
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4
SENT = (0, 1, 2, 0, 1, 2, 0, 1)     # the sentence of each of the B = 8 rows
B8 = len(SENT)


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


def batch(sent=SENT):
    src, m = D.make_src()
    idx = list(sent)
    return src[idx], m[idx]


def mixes():
    """Two B = 8 tables.  A: the step faults — linear INPUT / WEIGHT / OUTPUT / INPUT16 in
    different layers and at different steps, rows 0 and 2 sharing step 2, rows 0 and 3 sharing
    step 2 and layer 2, a self-attention fault on key 5 of 6 (inside a 4-key group), a cross
    attention fault on the padded sentence's neighbour, a row without a trial and a row whose
    step the decode never runs.  B: upsets of all four caches, codes and scales, next to step
    faults at the same steps (an upset and a step fault at step 3 and at step 4; step 2 with
    upsets alone), a linear WEIGHT16 and a QK^T output replacement."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    a = [(F("INPUT", 1, 2, "V", row=0, col=50, bit=7), 2),
         (F("WEIGHT", 1, 1, "K", row=77, col=300, bit=7), 0),
         (F("OUTPUT", 1, 0, "FFN2", row=0, col=100, value=3.0e4), 2),
         (F("INPUT16", 1, 2, "O", row=0, col=40, bit=7, win_start=32, win_len=16), 2),
         (F("WEIGHT", 1, 2, "PV", row=5, col=2 * 64 + 7, bit=7), 5),
         (F("INPUT", 1, 1, "CQK", row=0, col=4 * 64 + 9, bit=7), 3),
         None,
         (F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4), L - 1)]
    b = [(U("self_k", 0, row=1, col=33, bit=7), 3),
         (U("self_v", 3, row=2, bit=31, field="scale"), 4),
         (U("cross_k", 0, row=4, col=10, bit=7), 2),
         (U("cross_v", 2, row=13, col=300, bit=7), 0),
         (U("cross_v", 1, row=5, bit=31, field="scale"), 2),
         (F("WEIGHT16", 1, 3, "FFN1", row=7, col=100, bit=7, win_start=0, win_len=1), 3),
         (F("RANDOM", 1, 0, "QK", row=0, col=3 * 5 + 2, value=1.0e4), 4),
         (U("self_v", 1, row=3, col=70, bit=7), 5)]
    return {"A": a, "B": b}


def decode(model, src, m, trials, max_len=L):
    from qtx.decode import greedy_decode_kvfault_trials
    return greedy_decode_kvfault_trials(model, src, m, max_len, 0, trials)


def same_record(r, want, step):
    if want is None:
        assert r is None
        return
    assert r is not None and r.step == step
    np.testing.assert_array_equal(r.golden_ids, want[0])
    np.testing.assert_array_equal(bits(r.golden_logp), bits(want[1]))
    np.testing.assert_array_equal(r.faulty_ids, want[2])
    np.testing.assert_array_equal(bits(r.faulty_logp), bits(want[3]))


def check(model, om, src, m, trials, max_len=L):
    exp = T.expect_rows(om, src, m, max_len, trials)
    ys, sc, recs = decode(model, src, m, trials, max_len)
    np.testing.assert_array_equal(ys, exp[0])
    assert sc.top_ids.dtype == np.int64 and sc.top_logp.dtype == np.float32
    np.testing.assert_array_equal(sc.top_ids, exp[1])
    np.testing.assert_array_equal(bits(sc.top_logp), bits(exp[2]))
    for b, tr in enumerate(trials):
        same_record(recs[b], exp[3][b], None if tr is None else tr[1])
    return exp


def changed_rows(om, src, m, exp, max_len=L):
    """The rows whose result differs from the golden decode, in the oracle's expectation."""
    gold = T.expect_rows(om, src, m, max_len, [None] * src.shape[0])
    return [b for b in range(src.shape[0])
            if not (np.array_equal(exp[0][b], gold[0][b]) and
                    np.array_equal(bits(exp[2][b]), bits(gold[2][b])))]


# =====================================================================================
# 1. B = 8 and B = 33 against the reference
# =====================================================================================
@pytest.mark.parametrize("mix", ["A", "B"])
def test_b8_matches_reference(torch, gpu_model, oracle_model, mix):
    src, m = batch()
    trials = mixes()[mix]
    exp = check(gpu_model, oracle_model, src, m, trials)
    # every applied trial does something to its own row, and some change tokens
    applied = [b for b, tr in enumerate(trials) if tr is not None and tr[1] < L - 1]
    assert changed_rows(oracle_model, src, m, exp) == applied
    gold = T.expect_rows(oracle_model, src, m, L, [None] * B8)
    assert any(not np.array_equal(exp[0][b], gold[0][b]) for b in applied)


# six memoised (sentence, trial) pairs: rows of the two tables above
PAIRS33 = (("A", 0), ("A", 1), ("A", 2), ("A", 4), ("B", 3), ("B", 7))


def test_b33_cycles_six_pairs(torch, gpu_model, oracle_model):
    """33 rows: the eager step's GEMM crosses its 32-row tile, the faulty rows repeat at 6 apart."""
    mx = mixes()
    sent = [SENT[PAIRS33[r % 6][1]] for r in range(33)]
    trials = [mx[PAIRS33[r % 6][0]][PAIRS33[r % 6][1]] for r in range(33)]
    src, m = batch(sent)
    check(gpu_model, oracle_model, src, m, trials)


# =====================================================================================
# 2. path selection
# =====================================================================================
@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_GRAPH_STEPS": 3}, {"QTX_UNFUSED": 1},
                                 {"QTX_DECODE_GROUPS": 2}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()) or "default")
def test_paths(torch, gpu_model, oracle_model, knob_env, env):
    """Eager fused steps, graphs of 3 steps, the unfused step (row-major values, the stack's
    attention kernels) and two sub-batch groups give the reference's rows."""
    for k, v in env.items():
        knob_env(k, v)
    src, m = batch()
    for trials in mixes().values():
        check(gpu_model, oracle_model, src, m, trials)


# =====================================================================================
# 3. against the library itself, isolation, a 4-bit model, the campaign helper
# =====================================================================================
def test_rows_equal_the_standalone_call(torch, gpu_model):
    """Row b equals qtx_greedy_decode_kvfault on sentence b alone (B = 1, scored form)."""
    from qtx.decode import greedy_decode_kvfault
    from qtx.fault import Fault
    src, m = batch()
    mx = mixes()
    for name, rows in (("A", (0, 2, 4)), ("B", (7,))):
        trials = mx[name]
        ys, sc, recs = decode(gpu_model, src, m, trials)
        for b in rows:
            what, step = trials[b]
            kw = {"fault": what} if isinstance(what, Fault) else {"upset": what}
            y1, s1 = greedy_decode_kvfault(gpu_model, src[b:b + 1], m[b:b + 1], L, 0, step=step,
                                           return_scores=True, **kw)
            np.testing.assert_array_equal(ys[b], y1[0])
            np.testing.assert_array_equal(sc.top_ids[b], s1.top_ids[0])
            np.testing.assert_array_equal(bits(sc.top_logp[b]), bits(s1.top_logp[0]))
            r1 = s1.fault_step
            same_record(recs[b], (r1.golden_ids[0], r1.golden_logp[0], r1.faulty_ids[0],
                                  r1.faulty_logp[0]), step)


def test_isolation(torch, gpu_model, oracle_model):
    """A token-changing trial on row 0 alone: every other row is the golden scored decode."""
    from qtx.decode import greedy_decode
    src, m = batch()
    from qtx.fault import Fault as F
    trials = [(F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4), 2)] + [None] * (B8 - 1)
    exp = check(gpu_model, oracle_model, src, m, trials)
    gold = T.expect_rows(oracle_model, src, m, L, [None] * B8)
    assert not np.array_equal(exp[0][0], gold[0][0])
    ys, sc, recs = decode(gpu_model, src, m, trials)
    gy, gs = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
    np.testing.assert_array_equal(ys[1:], gy[1:])
    np.testing.assert_array_equal(sc.top_ids[1:], gs.top_ids[1:])
    np.testing.assert_array_equal(bits(sc.top_logp[1:]), bits(gs.top_logp[1:]))
    assert not np.array_equal(ys[0], gy[0]) and recs[1:] == [None] * (B8 - 1)


def test_4bit_model(torch):
    """Upsets do not depend on the weight width; a step fault on 4-bit weights is refused."""
    from model_cfgs import small_src, small_state
    from qtx._lib import QtxError
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    from qtx.model import QtxModel
    cfg, sd, om = small_state(512, 4, 97)
    model = QtxModel(sd, cfg)
    src, m = small_src(3, 9, 17, full=(0,))
    trials = [(U("cross_k", 0, row=3, col=5, bit=7), 1), None, (U("self_v", 1, row=1, col=70, bit=7), 3)]
    exp = check(model, om, src, m, trials)
    assert changed_rows(om, src, m, exp) == [0, 2]
    with pytest.raises(QtxError) as e:
        decode(model, src, m, [None, (F("INPUT", 1, 2, "FFN1", row=0, col=100, bit=6), 3), None])
    assert e.value.code == E_UNSUPPORTED and "row 1" in str(e.value)


def test_campaign_helper(torch, gpu_model, oracle_model):
    """Five trials on sentence 1 in batches of 4 (the second batch padded): the caller's order."""
    from qtx.decode import kvfault_campaign
    src, m = D.make_src()
    mx = mixes()
    trials = [mx["A"][1], mx["A"][4], mx["B"][7], mx["B"][1], mx["B"][4]]
    out = kvfault_campaign(gpu_model, src[1], m[1], L, trials, batch=4)
    assert len(out) == 5
    for (ys, sc, rec), tr in zip(out, trials):
        want = T.expect_row(oracle_model, src[1:2], m[1:2], L, tr)
        np.testing.assert_array_equal(ys, want[0])
        np.testing.assert_array_equal(sc.top_ids, want[1])
        np.testing.assert_array_equal(bits(sc.top_logp), bits(want[2]))
        same_record(rec, want[3], tr[1])
    assert kvfault_campaign(gpu_model, src[1], m[1], L, [], batch=4) == []


# =====================================================================================
# 4. extents and refusals
# =====================================================================================
def c_trials(trials):
    from qtx import _lib
    from qtx.fault import Fault
    arr = (_lib.KvTrial * len(trials))()
    for b, tr in enumerate(trials):
        if tr is None:
            continue
        what, arr[b].step = tr[0], int(tr[1])
        if isinstance(what, Fault):
            arr[b].what, arr[b].fault = 1, what.to_c()
        else:
            arr[b].what, arr[b].upset = 2, what.to_c()
    return arr


def _dev_inputs(torch):
    src, m = batch()
    return (torch.from_numpy(src).cuda(),
            torch.from_numpy(m.reshape(B8, S).astype(np.uint8)).cuda())


def _outs(torch, poison):
    spec = (((B8, L), torch.int64, "ids"), ((B8, L - 1, 2), torch.int64, "top_ids"),
            ((B8, L - 1, 2), torch.float32, "top_logp"), ((B8, 2, 2), torch.int64, "rec_ids"),
            ((B8, 2, 2), torch.float32, "rec_logp"))
    pairs = [guarded(torch, shp, dt, poison, name=n) for shp, dt, n in spec]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def rec_arrays(exp):
    """The record as the C entry writes it: [B, 2, 2], zeros for a row without an applied trial."""
    ri, rl = np.zeros((len(exp[3]), 2, 2), np.int64), np.zeros((len(exp[3]), 2, 2), np.float32)
    for b, r in enumerate(exp[3]):
        if r is not None:
            ri[b, 0], rl[b, 0], ri[b, 1], rl[b, 1] = r
    return ri, rl


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
def test_extents(torch, gpu_model, oracle_model, poison):
    """Exactly ids, top_ids, top_logp, rec_ids, rec_logp are written, each in full (the record
    rows of the golden rows as zeros); the workspace is not overrun; a short one is refused."""
    from qtx import _lib
    L_ = _lib.lib()
    trials = mixes()["A"]
    src, m = batch()
    exp = T.expect_rows(oracle_model, src, m, L, trials)
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_kvtrials_workspace_size(gpu_model.handle, B8, S, L)
    assert need > L_.qtx_greedy_kvfault_workspace_size(gpu_model.handle, B8, S, L)
    outs, checks = _outs(torch, poison)
    ws, cws = guarded(torch, (need,), torch.uint8, poison, name="workspace")
    head = (gpu_model.handle, P(srcd), P(md), B8, S, L, 0)
    arr = c_trials(trials)
    assert L_.qtx_greedy_decode_kvtrials(*head, *[P(t) for t in outs], P(ws), need - 1, arr,
                                         S0) == E_WORKSPACE
    torch.cuda.synchronize()
    for t in outs + [ws]:
        assert bool((t.view(torch.uint8) == poison).all())
    _lib.call("qtx_greedy_decode_kvtrials", *head, *[P(t) for t in outs], P(ws), need, arr, S0)
    gpu_model.check()
    for c in checks + [cws]:
        c()
    ids, ti, tl, ri, rl = outs
    wri, wrl = rec_arrays(exp)
    np.testing.assert_array_equal(ids.cpu().numpy(), exp[0])
    np.testing.assert_array_equal(ti.cpu().numpy(), exp[1])
    np.testing.assert_array_equal(bits(tl.cpu().numpy()), bits(exp[2]))
    np.testing.assert_array_equal(ri.cpu().numpy(), wri)
    np.testing.assert_array_equal(bits(rl.cpu().numpy()), bits(wrl))
    # top_ids / top_logp NULL: not copied out; without a record: ids alone
    outs2, checks2 = _outs(torch, poison)
    _lib.call("qtx_greedy_decode_kvtrials", *head, P(outs2[0]), S0, S0, P(outs2[3]), P(outs2[4]),
              P(ws), need, arr, S0)
    _lib.call("qtx_greedy_decode_kvtrials", *head, P(outs2[0]), S0, S0, S0, S0, P(ws), need, arr, S0)
    gpu_model.check()
    for c in checks2 + [cws]:
        c()
    np.testing.assert_array_equal(outs2[0].cpu().numpy(), exp[0])
    for t in outs2[1:3]:
        assert bool((t.view(torch.uint8) == poison).all())
    np.testing.assert_array_equal(outs2[3].cpu().numpy(), wri)
    np.testing.assert_array_equal(bits(outs2[4].cpu().numpy()), bits(wrl))


def test_refusals(torch, gpu_model):
    """Each refusal returns its status before anything is launched — the outputs and the
    workspace keep their poison — and names the row."""
    from qtx import _lib
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    L_ = _lib.lib()
    srcd, md = _dev_inputs(torch)
    need = L_.qtx_greedy_kvtrials_workspace_size(gpu_model.handle, B8, S, L)
    outs, checks = _outs(torch, 0x5A)
    ws, cws = guarded(torch, (need,), torch.uint8, 0x5A, name="workspace")
    head = (gpu_model.handle, P(srcd), P(md), B8, S, L, 0)

    def raw(arr, outs_=None, nbytes=need):
        rc = L_.qtx_greedy_decode_kvtrials(*head, *[P(t) for t in (outs_ or outs)], P(ws), nbytes,
                                           arr, S0)
        torch.cuda.synchronize()
        if rc != OK:
            for t in outs + [ws]:
                assert bool((t.view(torch.uint8) == 0x5A).all())
            for c in checks + [cws]:
                c()
        return rc

    def call(trial, row=5, nbytes=need):
        trials = [None] * B8
        trials[row] = trial
        rc = raw(c_trials(trials), nbytes=nbytes)
        if rc not in (OK, E_WORKSPACE):
            assert f"row {row}" in L_.qtx_last_error().decode()
        return rc

    good_f = F("INPUT", 1, 2, "FFN1", row=0, col=100, bit=6)
    good_u = U("self_k", 0, row=1, col=33, bit=7)
    assert raw(None) == E_INVALID                                     # trials NULL
    assert raw(c_trials([None] * B8), outs_=outs[:3] + [outs[3], None]) == E_INVALID   # half a record
    bad = c_trials([None] * B8)
    bad[2].what = 3
    assert raw(bad) == E_INVALID and "row 2" in L_.qtx_last_error().decode()
    assert call((good_f, -1)) == E_INVALID
    assert call((good_u, -1)) == E_INVALID
    assert call((F("INPUT", 0, 2, "FFN1", row=0, col=100, bit=6), 3)) == E_INVALID
    assert call((F("NONE", 1, 2, "FFN1"), 3)) == E_INVALID
    # B = 1 coordinates: the token row is 0, a linear WEIGHT16 window the one row, self keys
    # step + 1, an upset's row a position of the sentence
    assert call((F("INPUT", 1, 2, "FFN1", row=1, col=100, bit=6), 3)) == E_INVALID
    assert call((F("OUTPUT", 1, 2, "K", row=0, col=512, value=1.0), 3)) == E_INVALID
    assert call((F("WEIGHT16", 1, 3, "FFN1", row=7, col=100, bit=7, win_start=0, win_len=2), 3)) == E_INVALID
    assert call((F("WEIGHT", 1, 0, "QK", row=4, col=5, bit=7), 3)) == E_INVALID
    assert call((F("INPUT", 1, 0, "PV", row=0, col=7 * 4 + 4, bit=7), 3)) == E_INVALID
    assert call((F("WEIGHT", 1, 6, "K", row=40, col=200, bit=7), 1)) == E_INVALID
    assert call((F("WEIGHT", 1, 1, "CK", row=40, col=200, bit=7), 0)) == E_UNSUPPORTED
    assert call((F("INPUT", 1, 0, "CV", row=3, col=17, bit=7), 0)) == E_UNSUPPORTED
    assert call((U("self_k", 0, row=3, col=33, bit=7), 3)) == E_INVALID          # j >= step
    assert call((U("self_k", 0, row=1 * L + 1, col=33, bit=7), 3)) == E_INVALID  # a batch row
    assert call((U("cross_v", 0, row=S, col=33, bit=7), 3)) == E_INVALID
    assert call((U("self_k", 0, row=1, bit=23, field="scale"), 3)) == E_INVALID
    assert call((U("self_k", 0, row=1, col=512, bit=7), 3)) == E_INVALID
    assert call((U("cross_k", 6, row=0, col=33, bit=7), 3)) == E_INVALID
    assert call((good_f, 3), nbytes=need - 1) == E_WORKSPACE
    assert call((good_u, 3), nbytes=need - 1) == E_WORKSPACE
    # the boundaries are accepted; a trial that is never applied is not checked
    assert call((F("WEIGHT", 1, 0, "QK", row=3, col=5, bit=7), 3), row=7) == OK
    assert call((U("self_k", 0, row=2, bit=22, field="scale"), 3), row=0) == OK
    assert call((U("cross_v", 0, row=S - 1, col=511, bit=7), 0)) == OK
    assert call((F("INPUT", 1, 2, "FFN1", row=1, col=100, bit=6), L - 1)) == OK
    gpu_model.check()
