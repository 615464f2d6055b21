"""The step-graph runner's cache (csrc/qtx_stepgraph.h), observed through
qtx_debug_graph_stats: how many graphs each decode driver captures, that a repeated call
captures nothing, and that a plan of two graph sizes survives the cache's eviction.

Every expected count follows from the chunking rules of include/qtx.h (the greedy decode: one
graph of the whole decode, or graphs of QTX_GRAPH_STEPS steps where that divides max_len - 1;
the fault and beam decodes: graphs of QTX_GRAPH_STEPS (default 8) steps and of one step); none
is measured.  Outputs are checked against the oracle (greedy_decode, tests/dfault_cases.py's
campaign loop, tests/beam_ref.py), never against the code under test alone.

The small d_ff 512 model of tests/beam_ref.py (two layers, 97 words), B = 2, S = 9.  Each test
builds its own model: its counters start at zero.  The model's scratch is sized once up front,
since the graphs are keyed by the workspace they were captured on.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
import dfault_cases as D  # noqa: E402
import model_cfgs as MC  # noqa: E402

pytestmark = pytest.mark.gpu
B, S = 2, 9
L_GREEDY, L_FAULT = 12, 24
LAST = L_FAULT - 1            # the fault decode's steps: 0 .. LAST - 1
TAG = "stepgraph"


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def oracle():
    return R.boosted_state(512)[2]


def sources():
    return MC.small_src(B, S, 5)


def fresh_model():
    from qtx.model import QtxModel
    cfg, sd, _ = R.boosted_state(512)
    gm = QtxModel(sd, cfg)
    gm.workspace(64 << 20)        # never regrown: every call carves the same memory
    assert stats(gm) == (0, 0)
    return gm


def stats(gm):
    """(entries, captures) of the model's graph cache."""
    from qtx import _lib
    e, c = C.c_int32(-1), C.c_int64(-1)
    _lib.call("qtx_debug_graph_stats", gm.handle, C.byref(e), C.byref(c))
    return e.value, c.value


def dev_inputs(torch):
    src, m = sources()
    return (torch.from_numpy(src).cuda(),
            torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda())


def out_fault(step):
    """An OUTPUT fault on the last layer's FFN2 at sentence 0's last position of step `step`
    (T = step + 1 tokens per sentence), as (Fault, target_inference_number)."""
    from qtx.fault import Fault
    T = step + 1
    return Fault("OUTPUT", 1, 1, "FFN2", row=0 * T + T - 1, col=7, value=3.0e4), T


def expect_trial(step):
    src, m = sources()
    f, tin = out_fault(step)
    return D.oracle_trial(oracle(), src, m, L_FAULT, f, tin, TAG)


def check_trial(got, exp):
    """ids, top-2 ids, log-prob bits and the fault step's record against the oracle's trial."""
    ids, top_ids, top_logp, rec_ids, rec_logp = (t.cpu().numpy() for t in got[:5])
    np.testing.assert_array_equal(ids, exp[0])
    np.testing.assert_array_equal(top_ids, exp[1])
    np.testing.assert_array_equal(bits(top_logp), bits(exp[2]))
    if exp[3] is not None:
        np.testing.assert_array_equal(rec_ids, np.stack([exp[3][0], exp[3][2]], 1))
        np.testing.assert_array_equal(bits(rec_logp), bits(np.stack([exp[3][1], exp[3][3]], 1)))


def fault_decode(gm, torch, step, ws=None):
    srcd, md = dev_inputs(torch)
    got = gm.greedy_dfault(srcd, md, out_fault(step)[0], step, max_len=L_FAULT, scores=True, ws=ws)
    gm.check()
    return got


def beam(gm, max_len, K=4):
    from qtx.decode import beam_decode
    src, m = sources()
    return beam_decode(gm, src, m, max_len, R.START, beam_size=K, eos=R.EOS, pad=R.PAD, n_best=K,
                       early_exit=False)


def check_beam(r, max_len, K=4):
    src, m = sources()
    ref = D.memo(("beam", TAG, max_len, K), lambda: R.beam_ref(oracle(), src, m, max_len, K))
    np.testing.assert_array_equal(r.hyp_ids, ref["hyp_ids"])
    np.testing.assert_array_equal(r.hyp_len, ref["hyp_len"])
    np.testing.assert_array_equal(bits(r.hyp_score), bits(ref["hyp_score"]))
    assert r.steps_run == max_len - 1


def test_greedy(torch, knob_env):
    """One graph of the whole decode, captured by the first call and replayed by every later
    one, fresh id / mask tensors included; two sub-batch groups capture one graph each."""
    gm = fresh_model()
    srcd, md = dev_inputs(torch)
    src, m = sources()
    want = oracle().greedy_decode(src, m, L_GREEDY)
    for n in range(2):
        ids = gm.greedy(srcd, md, L_GREEDY, 0)
        assert stats(gm) == (1, 1), n
        np.testing.assert_array_equal(ids.cpu().numpy(), want)
    ids = gm.greedy(srcd.clone(), md.clone(), L_GREEDY, 0)
    assert stats(gm) == (1, 1)
    np.testing.assert_array_equal(ids.cpu().numpy(), want)
    knob_env("QTX_DECODE_GROUPS", 2)
    ids = gm.greedy(srcd, md, L_GREEDY, 0)
    assert stats(gm) == (2, 3)
    np.testing.assert_array_equal(ids.cpu().numpy(), want)
    gm.greedy(srcd, md, L_GREEDY, 0)
    assert stats(gm) == (2, 3)


def test_plain_and_scored_share_nothing_and_recapture_nothing(torch):
    gm = fresh_model()
    srcd, md = dev_inputs(torch)
    src, m = sources()
    want = oracle().greedy_decode(src, m, L_GREEDY)
    seen = []
    for scored in (False, True, False, True):
        out = gm.greedy(srcd, md, L_GREEDY, 0, scores=scored)
        np.testing.assert_array_equal((out[0] if scored else out).cpu().numpy(), want)
        seen.append(stats(gm))
    assert seen == [(1, 1), (2, 2), (2, 2), (2, 2)]


def test_fault_sweep(torch):
    """The scored fault decode at fault step 3, then resumes at fault steps 1, 5, 14 and 22:
    one 8-step and one 1-step graph serve them all.  A resume takes a fault step inside the
    workspace's golden prefix, which the decode at step 3 ends at step 3: the resume at 1
    follows it directly, and a never-applied fault decode (fault step 23: a golden decode,
    23 = 2 * 8 + 7 steps) on the same workspace gives the later resumes their prefix."""
    gm = fresh_model()
    ws = gm.dfault_workspace(B, S, L_FAULT)
    # steps 0 .. 3 are four replays of the 1-step graph, steps 4 .. 22 two 8-step graphs and
    # three more single steps
    check_trial(fault_decode(gm, torch, 3, ws), expect_trial(3))
    assert stats(gm) == (2, 2)
    reran = 0
    for order in ((1,), None, (22, 14, 5, 1)):
        if order is None:
            check_trial(fault_decode(gm, torch, LAST, ws), expect_trial(LAST))
            assert stats(gm) == (2, 2)
            continue
        for step in order:
            exp = expect_trial(step)
            got = gm.greedy_dfault_resume(ws, B, S, out_fault(step)[0], step, max_len=L_FAULT)
            gm.check()
            assert stats(gm) == (2, 2), step
            check_trial(got, exp)
            np.testing.assert_array_equal(got[5] != 0, exp[3][0][:, 0] != exp[3][2][:, 0])
            reran += bool(D.changed(exp)) and step + 1 < LAST
    assert reran >= 3      # (the oracle's verdict) resumes that ran the steps above the fault again


def test_beam(torch, knob_env):
    """max_len 12: 11 steps = one 8-step graph + three replays of the 1-step graph; with
    QTX_GRAPH_STEPS=3: 3 + 3 + 3 + 2, a 3-step graph and two replays of a 1-step graph."""
    gm = fresh_model()
    for n in range(2):
        check_beam(beam(gm, L_GREEDY), L_GREEDY)
        assert stats(gm) == (2, 2), n
    knob_env("QTX_GRAPH_STEPS", 3)
    for n in range(2):
        check_beam(beam(gm, L_GREEDY), L_GREEDY)
        assert stats(gm) == (4, 4), n


def test_eviction_inside_a_two_size_plan(torch):
    """Beam shapes fill the cache to 15 entries; the fault decode then needs two graph sizes,
    which do not both fit under the cap of 16: it gives what a fresh model gives."""
    from qtx.decode import greedy_decode
    gm = fresh_model()
    src, m = sources()
    before = greedy_decode(gm, src, m, L_GREEDY, 0)
    np.testing.assert_array_equal(before, oracle().greedy_decode(src, m, L_GREEDY))
    # max_len 4 .. 9: one graph each (1-step, or the 8-step one alone); 10 .. 13: two each
    for ml in range(4, 14):
        beam(gm, ml, K=2)
        assert stats(gm)[0] <= 16
    assert stats(gm)[0] == 15
    got = fault_decode(gm, torch, 3)
    assert stats(gm)[0] <= 16
    want = fault_decode(fresh_model(), torch, 3)
    for a, b in zip(got[:3], want[:3]):      # ids, top-2 ids, log-probabilities (bits)
        np.testing.assert_array_equal(a.cpu().numpy().view(np.int64 if a.dtype == torch.int64 else np.uint32),
                                      b.cpu().numpy().view(np.int64 if b.dtype == torch.int64 else np.uint32))
    check_trial(got, expect_trial(3))
    np.testing.assert_array_equal(greedy_decode(gm, src, m, L_GREEDY, 0), before)
    assert stats(gm)[0] <= 16


def test_eager_captures_nothing(torch, knob_env):
    knob_env("QTX_NO_GRAPH", 1)
    gm = fresh_model()
    srcd, md = dev_inputs(torch)
    src, m = sources()
    np.testing.assert_array_equal(gm.greedy(srcd, md, L_GREEDY, 0).cpu().numpy(),
                                  oracle().greedy_decode(src, m, L_GREEDY))
    assert stats(gm) == (0, 0)
    check_trial(fault_decode(gm, torch, 3), expect_trial(3))
    assert stats(gm) == (0, 0)
    check_beam(beam(gm, L_GREEDY), L_GREEDY)
    assert stats(gm) == (0, 0)
