"""The beam-search reference (tests/beam_ref.py) on the CPU: it reduces to the oracle's greedy
decode at beam 1, its inputs exercise what the GPU tests rely on, and the ranking helper.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
from model_cfgs import small_state  # noqa: E402

f32 = np.float32


def first_eos_cut(ys, eos, pad):
    """ys [B, L] with everything after each row's first EOS (past column 0) replaced by pad."""
    out = np.array(ys, copy=True)
    for row in out:
        hit = np.nonzero(row[1:] == eos)[0]
        if hit.size:
            row[hit[0] + 2:] = pad
    return out


def test_beam1_is_greedy_up_to_eos():
    cfg, sd, om = R.boosted_state(512)
    src, mask = R.inputs()
    ref = R.reference(512, 8, 97, 1)
    ys = om.greedy_decode(src, mask, R.MAX_LEN)
    np.testing.assert_array_equal(ref["hyp_ids"][:, 0], first_eos_cut(ys, R.EOS, R.PAD))
    # the lengths: up to and including the first EOS, else every step
    for b in range(src.shape[0]):
        hit = np.nonzero(ys[b, 1:] == R.EOS)[0]
        assert ref["hyp_len"][b, 0] == (hit[0] + 1 if hit.size else R.MAX_LEN - 1)
    assert ref["fin"][:, 0].any() and not ref["fin"][:, 0].all()


def test_beam1_unboosted_is_greedy_everywhere():
    _, _, om = small_state(512)
    src, mask = R.inputs()
    ys = om.greedy_decode(src, mask, R.MAX_LEN)
    assert not (ys[:, 1:] == R.EOS).any()        # no EOS: nothing is cut
    ref = R.beam_ref(om, src, mask, R.MAX_LEN, 1)
    np.testing.assert_array_equal(ref["hyp_ids"][:, 0], ys)
    assert ref["steps_run"] == R.MAX_LEN - 1 and (ref["hyp_len"] == R.MAX_LEN - 1).all()


@pytest.mark.parametrize("d_ff,bits,V,beam", [m for m in R.MODELS if m[3] > 1])
def test_inputs_exercise_the_search(d_ff, bits, V, beam):
    """What the GPU == reference comparison relies on, for every model it runs."""
    ref = R.reference(d_ff, bits, V, beam)
    total = R.MAX_LEN - 1
    fins = np.stack(ref["fins"])                 # [steps, B, K]
    pars = np.stack(ref["parents"])
    steps = fins.shape[0]
    ident = np.arange(beam)
    assert any(fins[:steps - 1, b].all(-1).any() for b in range(fins.shape[1])), \
        "no sentence has all hypotheses finished before the last step"
    assert not ref["fin"].all(-1).all(), "no sentence has an unfinished hypothesis at the end"
    nonid = sum(bool((pars[t] != ident).any()) for t in range(steps))
    assert 2 * nonid >= steps, f"parent vector non-identity at {nonid} of {steps} steps"
    assert any(len(set(p.tolist())) < beam for t in range(steps) for p in pars[t]), \
        "no two slots ever share a parent"
    # a finished hypothesis carried across at least 3 steps: finished, then selected again
    carried, c = 0, np.zeros(fins.shape[1:], np.int64)
    for t in range(1, steps):
        pfin = np.take_along_axis(fins[t - 1], pars[t], 1)    # the parent was finished already
        c = np.where(pfin, np.take_along_axis(c, pars[t], 1) + 1, 0)
        carried = max(carried, int(c.max()))
    assert carried >= 3, f"a finished hypothesis is carried across {carried} steps only"
    assert steps == ref["steps_run"] <= total


@pytest.mark.parametrize("d_ff,bits,V,beam", [m for m in R.MODELS if m[3] == 4 and m[2] == 97])
def test_two_sentence_batch_stops_early(d_ff, bits, V, beam):
    full = R.reference(d_ff, bits, V, beam)
    rows = R.early_rows(full)
    assert rows == (0, 2) if d_ff == 512 and bits == 8 else len(rows) >= 1
    ref = R.reference(d_ff, bits, V, beam, rows=rows)
    assert ref["steps_run"] < R.MAX_LEN - 1 and ref["fin"].all()
    # and it is the sub-batch of the full one (sentences are independent)
    np.testing.assert_array_equal(ref["hyp_ids"], full["hyp_ids"][list(rows)])
    np.testing.assert_array_equal(ref["hyp_score"], full["hyp_score"][list(rows)])


def test_select_ref_rules():
    V, pad = 7, 2
    logp = np.log(np.full((3, V), 1 / V, f32)).astype(f32)
    score = np.array([0, 0, -1], f32)
    par, tok, val = R.select_ref(score, np.zeros(3, bool), logp, pad)
    assert par.tolist() == [0, 0, 0] and tok.tolist() == [0, 1, 2]      # ties: smaller flat
    fin = np.array([False, True, False])
    par, tok, val = R.select_ref(score, fin, logp, pad)
    assert (par[0], tok[0], val[0]) == (1, pad, f32(0))                  # finished: score kept
    lp = logp.copy()
    lp[0] = np.nan
    par, tok, val = R.select_ref(np.array([0, -np.inf, -np.inf], f32), np.zeros(3, bool), lp, pad)
    assert par.tolist() == [0, 0, 0] and np.isneginf(val).all()          # NaN -> -inf, flat order


def test_rank_helper():
    from qtx.decode import rank_hypotheses
    score = np.array([[-1.0, -1.5, -1.5, -4.0]], f32)
    length = np.array([[2, 6, 6, 8]], np.int32)
    order, s = rank_hypotheses(score, length, 0.0)
    assert order.tolist() == [[0, 1, 2, 3]]                               # the library's order
    np.testing.assert_array_equal(s, score.astype(np.float64))
    order, s = rank_hypotheses(score, length, 1.0)                        # -0.5 -0.25 -0.25 -0.5
    assert order.tolist() == [[1, 2, 0, 3]]                               # reordered; ties stable
    np.testing.assert_array_equal(order, R.rank(score, length, 1.0))
    order, _ = rank_hypotheses(np.array([[-2.0, -2.0]], f32), np.array([[0, 3]], np.int32), 1.0)
    assert order.tolist() == [[1, 0]]                                     # max(len, 1)
