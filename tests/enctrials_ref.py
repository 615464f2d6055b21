"""The contract of qtx_greedy_decode_enctrials (include/qtx_enctrials.h): one independent
encoder-side fault trial per sentence of a batch, on the oracle (a helper module, not a conftest).

Row b of the batched call equals the stand-alone decode of sentence b ALONE with the row's fault
in that decode's coordinates.  An encoder fault (module 0) goes through the oracle's own
encode(fault=), then the KV-cached decode of tests/kvfault_ref.py over all steps; a memory K/V
projection fault (module 1, CK / CV) is tests/kvfault_ref.py's trial at step 0.  Nothing here
restates the decode.  Results are memoised per (sentence, fault).

cases() holds the two B = 8 tables the CPU and the GPU tests share, with the rows each lists as
applied; tests/test_enctrials_ref.py asserts on the oracle that those rows do change.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import kvfault_ref as R  # noqa: E402
from kvtrials_ref import _tag  # noqa: E402
from oracle.qtx_oracle import DecodeState  # noqa: E402

S, L = D.S, D.L
SENT = (0, 1, 2, 0, 1, 2, 0, 1)     # the sentence of each of the B = 8 rows


def expect_row(om, src1, m1, max_len, fault):
    """(ys [max_len], top_ids [max_len-1, 2], top_logp [max_len-1, 2]) of the one-sentence decode
    of src1 [1, S] / m1 [1, 1, S] with `fault`: None or a qtx.fault.Fault."""
    tag = _tag(src1, m1)
    if fault is None:
        g = R.golden(om, src1, m1, max_len, tag)
        return g["ys"][0], g["top_ids"][0], g["top_logp"][0]
    if fault.module == 1:
        assert fault.linear in ("CK", "CV")
        exp = R.trial(om, src1, m1, max_len, tag, fault=fault, step_i=0)
        return exp[0][0], exp[1][0], exp[2][0]

    def run():
        src_ = np.asarray(src1)
        memory = om.encode(om.embed(src_, om.src_lut), m1, fault=fault.as_dict())
        st = DecodeState(om, memory, m1, max_len)
        ys, ti, tv = R._run(om, st, np.zeros((1, 1), np.int64), 0, max_len - 1)
        return ys[0], np.stack(ti, 1)[0], np.stack(tv, 1)[0]
    return D.memo(("enctrial", tag, max_len, repr(fault)), run)


def expect_rows(om, src, m, max_len, faults):
    """The expectation of a batched call, row by row: (ys [B, max_len], top_ids, top_logp
    [B, max_len-1, 2])."""
    src, m = np.asarray(src), np.asarray(m)
    assert len(faults) == src.shape[0]
    rows = [expect_row(om, src[b:b + 1], m[b:b + 1], max_len, faults[b]) for b in range(len(faults))]
    return tuple(np.stack([r[k] for r in rows]) for k in range(3))


def batch(sent=SENT):
    src, m = D.make_src()
    idx = list(sent)
    return src[idx], m[idx]


def cases():
    """name -> (faults [8] for the sentences SENT, the rows listed as applied).  Between them:
    every encoder linear, QK and PV, CK and CV, all five kinds, golden rows; A rows 0 and 3 (a
    WEIGHT and an INPUT) and B rows 4 and 5 share a layer and a GEMM launch; A row 7 faults a
    padded token of sentence 1 (its 9 tokens end at row 8), which nothing downstream reads; B
    row 5 is a WEIGHT16 whose effect the quantizers absorb: both stay golden, not applied."""
    from qtx.fault import Fault as F
    a = [F("WEIGHT", 0, 1, "K", row=77, col=300, bit=7),
         F("OUTPUT", 0, 0, "FFN2", row=5, col=100, value=3.0e4),
         F("RANDOM", 0, 4, "QK", row=2, col=3 * S + 2, value=1.0e4),
         F("INPUT", 0, 1, "V", row=3, col=50, bit=7),
         F("INPUT", 1, 1, "CV", row=4, col=17, bit=7),
         None,
         F("INPUT16", 0, 5, "O", row=2, col=40, bit=7, win_start=32, win_len=16),
         F("INPUT", 0, 0, "Q", row=11, col=5, bit=7)]
    b = [F("OUTPUT", 0, 5, "FFN2", row=3, col=100, value=-2.0e4),
         F("WEIGHT", 0, 2, "PV", row=5, col=2 * 64 + 7, bit=7),
         F("WEIGHT", 1, 0, "CK", row=40, col=200, bit=7),
         F("INPUT", 0, 0, "Q", row=0, col=0, bit=0),
         F("INPUT", 0, 3, "FFN1", row=2, col=100, bit=7),
         F("WEIGHT16", 0, 3, "FFN1", row=7, col=100, bit=7, win_start=0, win_len=9),
         F("WEIGHT", 0, 4, "O", row=10, col=20, bit=7),
         F("INPUT16", 0, 3, "K", row=1, col=9, bit=7, win_start=100, win_len=16)]
    return {"A": (a, [0, 1, 2, 3, 4, 6]), "B": (b, [0, 1, 2, 3, 4, 6, 7])}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def changed_rows(om, src, m, exp, max_len=L):
    """The rows whose expectation differs from the golden decode's."""
    gold = expect_rows(om, src, m, max_len, [None] * src.shape[0])
    return [b for b in range(src.shape[0])
            if not (np.array_equal(exp[0][b], gold[0][b]) and np.array_equal(exp[1][b], gold[1][b])
                    and np.array_equal(bits(exp[2][b]), bits(gold[2][b])))]
