"""The premise and the tables of the encoder trials decode, on the oracle (CPU).

Premise: sentences of a batch never interact, so a B = 3 encode + decode with a fault in batch
coordinates gives, on the faulted sentence's row, the one-sentence run of tests/enctrials_ref.py.
Tables: every trial tests/enctrials_ref.py lists as applied changes its row's top_logp bits
against the golden row, at least three change tokens, every expected top_logp is finite, and the
rows not listed stay golden — so the GPU tests cannot pass vacuously."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import enctrials_ref as T  # noqa: E402
import kvfault_ref as R  # noqa: E402
from oracle.qtx_oracle import DecodeState  # noqa: E402

S, L = T.S, T.L


def _batch_run(om, src, m, fault):
    """The B = 3 decode with `fault` (batch coordinates) in the encoder or the memory K/V."""
    if fault.module == 1:
        exp = R.trial(om, src, m, L, "enctrials-b3", fault=fault, step_i=0)
        return exp[0], exp[1], exp[2]
    memory = om.encode(om.embed(src, om.src_lut), m, fault=fault.as_dict())
    st = DecodeState(om, memory, m, L)
    ys, ti, tv = R._run(om, st, np.zeros((src.shape[0], 1), np.int64), 0, L - 1)
    return ys, np.stack(ti, 1), np.stack(tv, 1)


def _premise_cases():
    from qtx.fault import Fault as F
    # (one-sentence fault, sentence b, the same fault in B = 3 batch coordinates)
    inp = F("INPUT", 0, 1, "V", row=3, col=50, bit=7)
    wgt = F("WEIGHT", 0, 1, "K", row=77, col=300, bit=7)
    pvw = F("WEIGHT", 0, 2, "PV", row=5, col=2 * 64 + 7, bit=7)
    ck = F("WEIGHT", 1, 0, "CK", row=40, col=200, bit=7)
    return {"input": (inp, 0, dataclasses.replace(inp, row=0 * S + 3)),
            "weight": (wgt, 2, wgt),
            "pv_weight": (pvw, 1, dataclasses.replace(pvw, row=1 * S + 5)),
            "ck_weight": (ck, 1, ck)}


@pytest.mark.parametrize("name", ["input", "weight", "pv_weight", "ck_weight"])
def test_batch_row_equals_the_one_sentence_run(oracle_model, name):
    f1, b, fb = _premise_cases()[name]
    src, m = D.make_src()
    ys, ti, tv = _batch_run(oracle_model, src, m, fb)
    want = T.expect_row(oracle_model, src[b:b + 1], m[b:b + 1], L, f1)
    np.testing.assert_array_equal(ys[b], want[0])
    np.testing.assert_array_equal(ti[b], want[1])
    np.testing.assert_array_equal(T.bits(tv[b]), T.bits(want[2]))


def test_tables_are_not_vacuous(oracle_model):
    src, m = T.batch()
    gold = T.expect_rows(oracle_model, src, m, L, [None] * len(T.SENT))
    tokens = 0
    for name, (faults, applied) in T.cases().items():
        exp = T.expect_rows(oracle_model, src, m, L, faults)
        assert np.isfinite(exp[2]).all(), name
        assert T.changed_rows(oracle_model, src, m, exp) == applied, name
        for b in applied:     # the scores change, not only the runner-up's id
            assert not np.array_equal(T.bits(exp[2][b]), T.bits(gold[2][b])), (name, b)
        tokens += sum(not np.array_equal(exp[0][b], gold[0][b]) for b in applied)
    assert tokens >= 3
    kinds = {f.kind for fs, _ in T.cases().values() for f in fs if f is not None}
    lins = {f.linear for fs, _ in T.cases().values() for f in fs if f is not None}
    assert {"INPUT", "WEIGHT", "INPUT16", "WEIGHT16"} <= kinds and kinds & {"OUTPUT", "RANDOM"}
    assert lins == {"Q", "K", "V", "O", "FFN1", "FFN2", "QK", "PV", "CK", "CV"}
