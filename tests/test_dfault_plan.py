"""The host side of the decoder-fault sweep: its visiting order and the public signatures
(no GPU)."""
import inspect
import os
import random
import re

import pytest


def test_plan_sweep_is_a_stable_descending_permutation():
    from qtx.decode import plan_sweep
    rnd = random.Random(5)
    cases = [[], [3], [1, 2, 2, 4, 6, 7, 70, 70], [5, 5, 5, 5], [0, 70, 0, 70, 1],
             [rnd.randrange(71) for _ in range(64)]]
    for steps in cases:
        order = plan_sweep(steps)
        assert sorted(order) == list(range(len(steps)))          # a permutation
        for a, b in zip(order, order[1:]):
            assert steps[a] > steps[b] or (steps[a] == steps[b] and a < b), (steps, order)


def test_plan_sweep_keeps_a_descending_list():
    from qtx.decode import plan_sweep
    assert plan_sweep([9, 7, 7, 3, 0]) == [0, 1, 2, 3, 4]
    assert plan_sweep([0, 3, 7, 7, 9]) == [4, 2, 3, 1, 0]


def test_public_signatures():
    import qtx
    from qtx import decode
    assert qtx.decode_fault_sweep is decode.decode_fault_sweep
    assert "decode_fault_sweep" in qtx.__all__
    p = inspect.signature(decode.decode_fault_sweep).parameters
    assert list(p) == ["model", "src", "src_mask", "max_len", "start_symbol", "trials"]
    p = inspect.signature(decode.greedy_decode_fault).parameters
    assert p["kv_cache"].default is False                         # the default path stays
    assert list(p)[-1] == "kv_cache" and list(p)[:5] == ["model", "src", "src_mask", "max_len",
                                                         "start_symbol"]
    assert list(inspect.signature(decode.plan_sweep).parameters) == ["steps"]
    s = decode.SweepStats()
    assert (s.n_trials, s.n_resumed, s.n_skipped) == (0, 0, 0)


def test_sweep_refuses_non_decoder_faults_before_touching_the_model():
    from qtx.decode import decode_fault_sweep
    from qtx.fault import Fault
    enc = Fault("INPUT", 0, 0, "Q", row=0, col=0, bit=1)
    for bad in ([(enc, 1)], [(None, 1)]):
        with pytest.raises(ValueError):
            decode_fault_sweep(None, None, None, 8, 0, bad)       # (the model is never reached)
    res, stats = decode_fault_sweep(None, None, None, 8, 0, [])
    assert res == [] and stats.n_trials == 0


def test_fault_step_of_a_target_inference_number():
    from qtx.decode import _fault_step
    L = 8
    assert [_fault_step(t, L) for t in (1, 2, L - 1)] == [0, 1, L - 2]
    # numbers the loop never reaches: a step that does not exist (never applied)
    assert [_fault_step(t, L) for t in (0, -3, L, L + 3)] == [L - 1] * 4


def test_header_declares_the_three_entry_points():
    from qtx import _lib
    names = ("qtx_greedy_dfault_workspace_size", "qtx_greedy_decode_dfault",
             "qtx_greedy_dfault_resume")
    syms = _lib.header_symbols()
    for n in names:
        assert n in syms and n in _lib.SIGNATURES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "include", "qtx.h")).read()
    for n in names[1:]:                                          # each cites the campaign loop
        assert re.search(n + r" \(:536-740", text), n
