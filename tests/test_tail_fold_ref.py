"""The folded decode tail's record merge, restated in numpy (tests/tail_fold_ref.py), against
argmax / sorted top-2 and the oracle's log_softmax_argmax on random rows with duplicates,
+-inf and NaN.  No GPU."""
import os
import sys

import numpy as np

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_fold_ref as R  # noqa: E402

f32 = np.float32


def rows(V, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(24):
        r = (rng.standard_normal(V) * 2).astype(f32)
        kind = k % 8
        j = rng.choice(V, size=min(4, V), replace=False)
        if kind == 1:
            r[j[:2]] = r.max() + f32(1)                    # the maximum twice
        elif kind == 2:
            r[j[0]] = r.max() + f32(1)
            r[j[1]] = np.nextafter(r[j[0]], f32(-np.inf))  # 1 ulp below the maximum
        elif kind == 3:
            r[j[0]] = -np.inf
            r[j[1]] = r.max() + f32(3)
        elif kind == 4:
            r[j[0]] = np.inf
        elif kind == 5:
            r[j[0]] = np.nan
            r[j[1]] = -np.inf
        elif kind == 6:
            r[:] = -np.inf
            if k > 8:
                r[j[0]] = f32(0.5)                          # one finite value
        elif kind == 7:
            r[:] = f32(1.25)                                # all equal
        out.append(r)
    r = np.full(V, -np.inf, f32)                            # the maximum in the last column
    r[V - 1] = 1.0
    out.append(r)
    return out


def test_records_and_merge_against_numpy():
    for V in (2, 16, 17, 97, 130, 1031):
        for r in rows(V, V):
            recs = R.strip_records(r)
            assert len(recs) == (V + 15) // 16
            m1, m2, i1, fl = R.merge_all(recs)
            # any merge order gives the same record (max / top-2 is order-free)
            perm = np.random.default_rng(V).permutation(len(recs))
            assert R.merge_all(recs, perm) == (m1, m2, i1, fl)
            half = len(recs) // 2
            tree = R.merge(R.merge_all(recs[:half]), R.merge_all(recs[half:]))
            assert tree == (m1, m2, i1, fl)
            c = np.fmax(R.NEG, r)
            assert m1 == c.max()
            eq = np.nonzero(r == m1)[0]
            assert i1 == (eq[0] if len(eq) else R.IMAX)
            srt = np.sort(c)[::-1]
            assert m2 == srt[1]                             # with multiplicity
            assert bool(fl & 1) == bool(np.isnan(r).any() or np.isposinf(r).any())
            assert bool(fl & 2) == bool((r > -np.inf).any())


def test_decision_against_oracle():
    seen = set()
    for V in (16, 97, 1031):
        for r in rows(V, 7 * V):
            kind, tok = R.decide(R.merge_all(R.strip_records(r)))
            seen.add(kind)
            _, ref = O.log_softmax_argmax(r[None])
            bad = np.isnan(r).any() or np.isposinf(r).any() or np.isneginf(r).all()
            assert (kind == "bad") == bool(bad)
            if kind != "exact":
                assert tok == ref[0]
            else:   # exactly the rows k_argmax_embed sends down its exact path
                mx = np.fmax(R.NEG, r).max()
                assert np.count_nonzero(r > f32(mx - R.DELTA)) != 1
    assert seen == {"bad", "fast", "exact"}
