"""What licenses tests/wide_batch.py's expansion, on the CPU: the expected rows of a 7-row batch
— per-sentence oracle results indexed by the cycle — equal the oracle run on those 7 rows as
one real batch, bit for bit, for the scored greedy decode, one kvtrials table and one beam
search.  The small two-layer d_ff 512 model of tests/beam_ref.py (tests/model_cfgs.py with the
EOS bias raised) and its sources; a few seconds in all.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import kvfault_ref as R  # noqa: E402
import wide_batch as W  # noqa: E402

B7, L = 7, 8
bits = W.bits


def setup():
    om = BR.boosted_state(512)[2]
    src3, m3 = BR.inputs()
    return om, src3[:W.CYCLE], m3[:W.CYCLE]


def test_cycle_and_placement():
    assert W.sentence_of(7) == [0, 1, 2, 0, 1, 2, 0]
    src3, m3 = W.D.make_src()
    src, m = W.default_batch(97)
    assert src.shape == (97, W.D.S) and m.shape == (97, 1, W.D.S)
    np.testing.assert_array_equal(src[96], src3[0])
    np.testing.assert_array_equal(m[95], m3[2])
    tab = W.place(13, [["a0", "a1"], ["b0"], ["c0", "c1", "c2"]], edges=(12,))
    # rows 2 and 7 stay empty, row 12 (an edge) does not; every sentence walks its own list
    assert tab == ["a0", "b0", None, "a1", "b0", "c0", "a0", None, "c1", "a1", "b0", "c2", "a0"]


def test_assert_distinct_sees_a_repeated_sentence():
    import pytest
    a = (np.arange(4), np.ones(3, np.float32))
    b = (np.arange(4), np.full(3, 1.0000001, np.float32))       # the log-probability bits differ
    c = (np.arange(1, 5), np.ones(3, np.float32))
    W.assert_distinct([a, b, c])
    with pytest.raises(AssertionError):
        W.assert_distinct([a, c, (np.arange(4), np.ones(3, np.float32))])


def test_scored_greedy_expansion():
    om, src3, m3 = setup()
    src, m = W.batch(src3, m3, B7)
    g = R.golden(om, src, m, L, "wide7")
    ys, ti, tv = W.golden_rows(om, src3, m3, B7, L)
    np.testing.assert_array_equal(ys, g["ys"])
    np.testing.assert_array_equal(ti, g["top_ids"])
    np.testing.assert_array_equal(bits(tv), bits(g["top_logp"]))
    np.testing.assert_array_equal(ys, om.greedy_decode(src, m, L))


def test_kvtrials_expansion():
    """Rows 0, 3, 4 and 6 (the last) carry a trial, in the coordinates of their sentence alone;
    the batch oracle runs each one in the batch's coordinates: its row equals the expanded
    reference's, every other row the golden batch decode."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    om, src3, m3 = setup()
    src, m = W.batch(src3, m3, B7)
    S = src.shape[1]
    trials = [(F("OUTPUT", 1, 1, "FFN2", row=0, col=100, value=3.0e4), 2), None, None,
              (U("self_v", 1, row=1, col=70, bit=7), 3),
              (F("INPUT", 1, 0, "V", row=0, col=50, bit=7), 2), None,
              (U("cross_k", 0, row=3, col=5, bit=7), 1)]
    ys, ti, tv, recs = W.kvtrials_rows(om, src3, m3, L, trials)
    g = R.golden(om, src, m, L, "wide7")
    changed = 0
    for b, tr in enumerate(trials):
        if tr is None:
            assert recs[b] is None
            np.testing.assert_array_equal(ys[b], g["ys"][b])
            np.testing.assert_array_equal(bits(tv[b]), bits(g["top_logp"][b]))
            continue
        what, step = tr
        wb = W.kv_to_batch(what, b, S, L)
        kw = {"fault": wb} if isinstance(what, F) else {"upset": wb}
        e = R.trial(om, src, m, L, "wide7", step_i=step, **kw)
        np.testing.assert_array_equal(e[0][b], ys[b])
        np.testing.assert_array_equal(e[1][b], ti[b])
        np.testing.assert_array_equal(bits(e[2][b]), bits(tv[b]))
        for k in (0, 2):
            np.testing.assert_array_equal(e[3][k][b], recs[b][k])
            np.testing.assert_array_equal(bits(e[3][k + 1][b]), bits(recs[b][k + 1]))
        others = [r for r in range(B7) if r != b]
        np.testing.assert_array_equal(e[0][others], g["ys"][others])
        np.testing.assert_array_equal(bits(e[2][others]), bits(g["top_logp"][others]))
        changed += not np.array_equal(bits(tv[b]), bits(g["top_logp"][b]))
        # and the one-row form the kvfault cases use
        ky, kti, ktv, krec = W.kvfault_rows(om, src3, m3, B7, L, b, what, step)
        np.testing.assert_array_equal(ky, e[0])
        np.testing.assert_array_equal(kti, e[1])
        np.testing.assert_array_equal(bits(ktv), bits(e[2]))
        for k in (0, 2):
            np.testing.assert_array_equal(krec[k], e[3][k])
            np.testing.assert_array_equal(bits(krec[k + 1]), bits(e[3][k + 1]))
    assert changed >= 3


def test_beam_expansion():
    om, src3, m3 = setup()
    src, m = W.batch(src3, m3, B7)
    real = BR.beam_ref(om, src, m, BR.MAX_LEN, 3)
    exp = W.beam_rows(lambda s: BR.reference(512, 8, 97, 3, rows=(s,)), B7)
    np.testing.assert_array_equal(exp["hyp_ids"], real["hyp_ids"])
    np.testing.assert_array_equal(exp["hyp_len"], real["hyp_len"])
    np.testing.assert_array_equal(bits(exp["hyp_score"]), bits(real["hyp_score"]))
    assert exp["steps_run"] == real["steps_run"]
    assert any(W.reorders(r) for r in exp["refs"])
    # the sentences do not all run the same number of steps: one finishes while the batch goes on
    assert min(r["steps_run"] for r in exp["refs"]) < real["steps_run"]
