"""The contract of qtx_greedy_decode_kvtrials (include/qtx.h): one independent kvfault trial per
sentence of a batch, on the oracle (a helper module, not a conftest).

Row b of the batched call equals the stand-alone trial on sentence b ALONE.  So the expectation
of a row is tests/kvfault_ref.py's trial() on src[b:b+1] with the row's fault or upset in the
coordinates of that one-sentence decode; nothing here restates the decode.  Results are
memoised per (sentence, trial): rows that repeat a sentence and a trial share one oracle run.

localize() moves a trial written for tests/kvfault_cases.py's B = 3 batch into the coordinates of
one of its sentences.
"""
import dataclasses
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kvfault_ref as R  # noqa: E402

ATTN = ("QK", "PV", "CQK", "CPV")


def _tag(src1, m1):
    h = hashlib.sha1(np.ascontiguousarray(src1).tobytes())
    h.update(np.ascontiguousarray(np.asarray(m1) != 0).tobytes())
    return "row:" + h.hexdigest()[:16]


def expect_row(om, src1, m1, max_len, trial):
    """(ys [max_len], top_ids [max_len-1, 2], top_logp [max_len-1, 2], record or None) of the
    one-sentence decode of src1 [1, S] / m1 [1, 1, S] with `trial`: None, or (Fault | CacheUpset,
    step) in that decode's coordinates.  record = (golden ids, golden logp, faulty ids, faulty
    logp), [2] each; None for a row without an applied trial."""
    from qtx.fault import Fault
    tag = _tag(src1, m1)
    if trial is None:
        g = R.golden(om, src1, m1, max_len, tag)
        return g["ys"][0], g["top_ids"][0], g["top_logp"][0], None
    what, step = trial
    if isinstance(what, Fault):
        exp = R.trial(om, src1, m1, max_len, tag, fault=what, step_i=int(step))
    else:
        exp = R.trial(om, src1, m1, max_len, tag, upset=what, step_i=int(step))
    rec = None if exp[3] is None else tuple(np.asarray(a)[0] for a in exp[3])
    return exp[0][0], exp[1][0], exp[2][0], rec


def expect_rows(om, src, m, max_len, trials):
    """The expectation of a batched call, row by row: (ys [B, max_len], top_ids, top_logp
    [B, max_len-1, 2], records [B] of record-or-None)."""
    src, m = np.asarray(src), np.asarray(m)
    assert len(trials) == src.shape[0]
    rows = [expect_row(om, src[b:b + 1], m[b:b + 1], max_len, trials[b]) for b in range(len(trials))]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.stack([r[2] for r in rows]), [r[3] for r in rows])


def localize(what, step, S, max_len, sentence=None):
    """A trial in the coordinates of a batch -> (sentence b, the trial in the coordinates of the
    decode of sentence b alone).  A linear WEIGHT fault has no sentence of its own (every row
    sees it): `sentence` names the one asked for; a linear WEIGHT16 window becomes the one row."""
    from qtx.fault import CacheUpset, Fault
    if isinstance(what, CacheUpset):
        b, j = divmod(int(what.row), max_len if what.cache.startswith("self") else S)
        return b, dataclasses.replace(what, row=j)
    assert isinstance(what, Fault)
    weight = what.kind in ("WEIGHT", "WEIGHT16")
    if what.linear in ATTN:
        if not weight:
            return int(what.row), dataclasses.replace(what, row=0)
        b, j = divmod(int(what.row), S if what.linear in ("CQK", "CPV") else step + 1)
        return b, dataclasses.replace(what, row=j)
    if not weight:
        return int(what.row), dataclasses.replace(what, row=0)
    assert sentence is not None
    if what.kind == "WEIGHT16":
        assert what.win_start <= sentence < what.win_start + what.win_len
        return sentence, dataclasses.replace(what, win_start=0, win_len=1)
    return sentence, what
