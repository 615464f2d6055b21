"""The premise of qtx_greedy_decode_kvtrials' contract, on the oracle (CPU only): sentences of a
batch never interact, so row b of a B = 3 kvfault trial (tests/kvfault_ref.py) equals, bit for
bit and including the record, the trial on sentence b alone in that sentence's own coordinates
(tests/kvtrials_ref.py).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import kvfault_cases as K  # noqa: E402
import kvfault_ref as R  # noqa: E402
import kvtrials_ref as T  # noqa: E402

L, S = D.L, D.S
# (case, the sentence a linear WEIGHT fault is looked at on)
CASES = (("in_v_l2_s2", None), ("out_ffn2_l0_s2", None), ("w_pv_s5_j5", None), ("up_sv_j3", None),
         ("up_cv_last", None), ("w_k_l1_s0", 2), ("w16_ffn1_s3", 1))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,sentence", CASES, ids=[c[0] for c in CASES])
def test_batch_row_equals_the_sentence_alone(oracle_model, name, sentence):
    src, m = D.make_src()
    f, u, step = K.cases()[name]
    what = f if f is not None else u
    big = R.trial(oracle_model, src, m, L, "main", f, u, step)
    b, one = T.localize(what, step, S, L, sentence)
    ys, ti, tl, rec = T.expect_row(oracle_model, src[b:b + 1], m[b:b + 1], L, (one, step))
    np.testing.assert_array_equal(ys, big[0][b])
    np.testing.assert_array_equal(ti, big[1][b])
    np.testing.assert_array_equal(bits(tl), bits(big[2][b]))
    assert rec is not None
    for got, want in zip(rec, big[3]):
        np.testing.assert_array_equal(bits(got) if got.dtype == np.float32 else got,
                                      bits(want[b]) if got.dtype == np.float32 else want[b])
    # the trial does something to this sentence (else the comparison says nothing)
    g = R.golden(oracle_model, src, m, L, "main")
    assert not (np.array_equal(ys, g["ys"][b]) and
                np.array_equal(bits(tl), bits(g["top_logp"][b])))


def test_a_row_without_a_trial_is_the_golden_decode(oracle_model):
    src, m = D.make_src()
    g = R.golden(oracle_model, src, m, L, "main")
    ys, ti, tl, recs = T.expect_rows(oracle_model, src, m, L, [None] * D.B)
    np.testing.assert_array_equal(ys, g["ys"])
    np.testing.assert_array_equal(ti, g["top_ids"])
    np.testing.assert_array_equal(bits(tl), bits(g["top_logp"]))
    assert recs == [None] * D.B
