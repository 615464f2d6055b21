"""numpy restatement of the folded decode tail's reduction (csrc/qtx_decode.hip: the per-strip
top-2 records k_generator_mfma writes, their merge and the decision in k_skinny_wide_tok),
shared by tests/test_tail_fold_ref.py (CPU) and tests/test_gpu_tail_fold.py (GPU)."""
import numpy as np

f32 = np.float32
NEG = f32(-3.0e38)
IMAX = 2 ** 31 - 1
DELTA = f32(4.0e-6)


def strip_records(row):
    """[V] logits -> list of (m1, m2, i1, flags), one per 16-column strip."""
    row = np.asarray(row, f32)
    out = []
    for s0 in range(0, len(row), 16):
        v = row[s0:s0 + 16]
        c = np.fmax(NEG, v)                                  # fmaxf: a NaN drops out
        m1 = c.max()
        eq = np.nonzero(v == m1)[0]
        i1 = s0 + int(eq[0]) if len(eq) else IMAX
        rest = np.delete(c, i1 - s0) if len(eq) else c
        m2 = rest.max() if len(rest) else NEG
        fl = (1 if (~(v < np.inf)).any() else 0) | (2 if (v > -np.inf).any() else 0)
        out.append((f32(m1), f32(m2), i1, fl))
    return out


def merge(a, b):
    """The record of the union of two disjoint sets."""
    lead = b[0] > a[0] or (b[0] == a[0] and b[2] < a[2])
    win, lose = (b, a) if lead else (a, b)
    return (win[0], max(a[1], b[1], lose[0]), win[2], a[3] | b[3])


def merge_all(recs, order=None):
    order = range(len(recs)) if order is None else order
    acc = (NEG, NEG, IMAX, 0)
    for i in order:
        acc = merge(acc, recs[i])
    return acc


def decide(rec):
    """('bad', 0) | ('fast', id) | ('exact', None) from a row's merged record."""
    m1, m2, i1, fl = rec
    if (fl & 1) or not (fl & 2):
        return "bad", 0
    if not (m2 > f32(m1 - DELTA)) and i1 != IMAX:
        return "fast", i1
    return "exact", None
