"""Wide batches for tests/test_gpu_wide_batch.py and their references (a helper module, not a
conftest): 33 to 200 rows, past the row-block switches of the decode step.

A wide batch is a cycle of CYCLE = 3 distinct sentences repeated over its rows: row r holds
sentence r % 3.  3 shares no factor with the 4-, 8-, 16- and 32-row blocks of the step's kernels,
so a row read one block off lands on another sentence, and assert_distinct() checks on the
oracle's results that another sentence means another result.

Expected values never come from the code under test.  The sentences of a batch are independent
(the contract of tests/kvtrials_ref.py and tests/enctrials_ref.py; tests/test_beam_ref.py shows it
for the beam reference), so the expectation of row r is the oracle's result for sentence r % 3
decoded ALONE, with the row's trial in that decode's coordinates, memoised per (sentence, trial):
the oracle decodes three sentences per case, not 193.  tests/test_wide_batch_ref.py checks the
expansion against the oracle run on a real 7-row batch, bit for bit.
"""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import enctrials_ref as ET  # noqa: E402
import kvtrials_ref as KT  # noqa: E402

CYCLE = 3
ATTN = KT.ATTN


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def sentence_of(B):
    """The sentence of each of the B rows."""
    return [r % CYCLE for r in range(B)]


def batch(src3, m3, B):
    """The first CYCLE sentences of src3 [>= 3, S] / m3 [>= 3, 1, S] cycled over B rows."""
    idx = sentence_of(B)
    return np.asarray(src3)[idx], np.asarray(m3)[idx]


def default_batch(B):
    """tests/dfault_cases.py's three sentences (S = 14, sentence 1 padded to 9) over B rows."""
    return batch(*D.make_src(), B)


def expand(per_sentence, B):
    """per_sentence: CYCLE tuples of arrays (one per sentence) -> the tuple of [B, ...] arrays."""
    idx = sentence_of(B)
    return tuple(np.stack([per_sentence[s][k] for s in idx]) for k in range(len(per_sentence[0])))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def assert_distinct(per_sentence):
    """The results of the cycle's sentences (tuples of arrays: ids, log-probabilities) are pairwise
    different in some array — ids, or log-probability bits.  Without that a swapped row would
    not show."""
    n = len(per_sentence)
    assert n == CYCLE
    for i in range(n):
        for j in range(i + 1, n):
            assert not all(_same(a, b) for a, b in zip(per_sentence[i], per_sentence[j])), \
                f"sentences {i} and {j} have the same result: a swapped row would not show"


def _one(src3, m3, s):
    return np.asarray(src3)[s:s + 1], np.asarray(m3)[s:s + 1]


# =====================================================================================
# greedy and scored greedy
# =====================================================================================
def golden_sentences(om, src3, m3, max_len):
    """[(ys [max_len], top_ids, top_logp [max_len-1, 2])] of each sentence decoded alone."""
    return [KT.expect_row(om, *_one(src3, m3, s), max_len, None)[:3] for s in range(CYCLE)]


def golden_rows(om, src3, m3, B, max_len):
    """The scored golden decode of the B-row batch: (ys [B, max_len], top_ids, top_logp)."""
    per = golden_sentences(om, src3, m3, max_len)
    assert_distinct(per)
    return expand(per, B)


# =====================================================================================
# kvtrials / enctrials: the references expand by row already
# =====================================================================================
def kvtrials_rows(om, src3, m3, max_len, trials):
    """tests/kvtrials_ref.expect_rows on the cycled batch; trials [B] in B = 1 coordinates."""
    src, m = batch(src3, m3, len(trials))
    return KT.expect_rows(om, src, m, max_len, trials)


def enctrials_rows(om, src3, m3, max_len, faults):
    src, m = batch(src3, m3, len(faults))
    return ET.expect_rows(om, src, m, max_len, faults)


def place(B, per_sentence, edges, skip=5):
    """A table of B entries: row r takes the next entry of per_sentence[r % 3] (each list is
    walked round and round), except the rows with r % skip == 2, which stay None — unless the
    row is one of `edges`, which always get an entry."""
    out, seen = [], [0] * CYCLE
    for r in range(B):
        s = r % CYCLE
        if r % skip == 2 and r not in edges:
            out.append(None)
            continue
        out.append(per_sentence[s][seen[s] % len(per_sentence[s])])
        seen[s] += 1
    return out


# =====================================================================================
# kvfault: one step fault or upset on one row of the batch
# =====================================================================================
def kv_to_batch(what, b, S, max_len):
    """A kvfault trial in the coordinates of sentence b alone -> the batch's coordinates (the
    inverse of tests/kvtrials_ref.localize for the kinds that name one row)."""
    from qtx.fault import CacheUpset
    if isinstance(what, CacheUpset):
        return dataclasses.replace(what, row=b * (max_len if what.cache.startswith("self") else S)
                                   + int(what.row))
    assert what.kind in ("INPUT", "INPUT16", "OUTPUT", "RANDOM") and int(what.row) == 0
    return dataclasses.replace(what, row=b)


def kvfault_rows(om, src3, m3, B, max_len, b, what, step):
    """qtx_greedy_decode_kvfault on the cycled batch with `what` (in the coordinates of its
    sentence alone) on row b at `step`: (ys, top_ids, top_logp, record); row b from
    tests/kvfault_ref.py on that sentence alone, every other row golden.  record = (golden ids,
    golden logp, faulty ids, faulty logp) [B, 2] each."""
    ys, ti, tv = (a.copy() for a in golden_rows(om, src3, m3, B, max_len))
    gi, gv = ti[:, step].copy(), tv[:, step].copy()
    row = KT.expect_row(om, *_one(src3, m3, b % CYCLE), max_len, (what, step))
    ys[b], ti[b], tv[b] = row[:3]
    fi, fv = gi.copy(), gv.copy()
    np.testing.assert_array_equal(row[3][0], gi[b])
    fi[b], fv[b] = row[3][2], row[3][3]
    return ys, ti, tv, (gi, gv, fi, fv)


# =====================================================================================
# dfault: the campaign's full-prefix faulty step on the last token of one row
# =====================================================================================
def dfault_to_batch(fault, b, tin):
    """A linear INPUT / OUTPUT fault on the last token (row tin - 1 of the one sentence's
    [tin] prefix rows) -> row b * tin + tin - 1 of the batch's [B * tin]."""
    assert fault.kind in ("INPUT", "OUTPUT") and fault.linear not in ATTN
    assert int(fault.row) == tin - 1
    return dataclasses.replace(fault, row=b * tin + tin - 1)


def dfault_rows(om, src3, m3, B, max_len, b, fault, tin):
    """qtx_greedy_decode_dfault / a resume on the cycled batch with `fault` (coordinates of its
    sentence alone) on row b: row b from tests/dfault_cases.oracle_trial on that sentence alone,
    every other row that oracle's golden decode.  (ys, top_ids, top_logp, record)."""
    per = []
    for s in range(CYCLE):
        src1, m1 = _one(src3, m3, s)
        _, gy, gi, gv = D.oracle_golden(om, src1, m1, max_len, KT._tag(src1, m1))
        per.append((gy[0], gi[0], gv[0]))
    assert_distinct(per)
    ys, ti, tv = (a.copy() for a in expand(per, B))
    step = tin - 1
    gi, gv = ti[:, step].copy(), tv[:, step].copy()
    src1, m1 = _one(src3, m3, b % CYCLE)
    ty, tti, ttv, rec = D.oracle_trial(om, src1, m1, max_len, fault, tin, KT._tag(src1, m1))
    ys[b], ti[b], tv[b] = ty[0], tti[0], ttv[0]
    fi, fv = gi.copy(), gv.copy()
    np.testing.assert_array_equal(rec[0][0], gi[b])
    fi[b], fv[b] = rec[2][0], rec[3][0]
    return ys, ti, tv, (gi, gv, fi, fv)


# =====================================================================================
# beam search
# =====================================================================================
def beam_rows(ref_of, B):
    """ref_of(s): tests/beam_ref.beam_ref's dict for sentence s alone -> the B-row batch's
    hyp_ids [B, K, max_len], hyp_score, hyp_len [B, K], steps_run (a batch runs until its last
    sentence has finished; a finished sentence's later steps change nothing: PAD tokens, the
    score and the length kept, the identity as parents) and the per-sentence dicts."""
    refs = [ref_of(s) for s in range(CYCLE)]
    assert_distinct([(r["hyp_ids"][0], r["hyp_score"][0], r["hyp_len"][0]) for r in refs])
    ids, score, length = expand([(r["hyp_ids"][0], r["hyp_score"][0], r["hyp_len"][0])
                                 for r in refs], B)
    return dict(hyp_ids=ids, hyp_score=score, hyp_len=length,
                steps_run=max(r["steps_run"] for r in refs), refs=refs)


def reorders(ref):
    """Whether some step's parents of a one-sentence beam reference are not the identity."""
    K = ref["hyp_ids"].shape[1]
    return any((p[0] != np.arange(K)).any() for p in ref["parents"])
