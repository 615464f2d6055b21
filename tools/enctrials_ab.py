#!/usr/bin/env python3
"""Wall time per encoder-side fault trial in one process at bench.py's shape and inputs (S = 72,
max_len = 72, the cfg2 model): 32 trials, one per sentence of bench.py's batch, drawn from a
fixed seed — linear encoder faults of every kind, encoder attention faults, and memory K/V
projection (CK / CV) faults.  In ms as the caller sees it, alternating in rounds so that clock
drift hits all alike:

  (a) 32 stand-alone B = 1 calls of the existing entries, one sentence each:
      greedy_decode_fault(return_scores=True) for an encoder fault,
      greedy_decode_kvfault(step=0, return_scores=True) for CK / CV
  (b) one greedy_decode_enctrials call on the 32 rows (qtx_greedy_decode_enctrials)
  (c) greedy_decode(return_scores=True) on the 32 rows: the scored golden decode

Before timing, every row of (b) is compared with its call of (a), bit for bit.  (b) - (c) is the
price of the row-major table encoder (and, with a CK / CV trial, the per-layer cross K/V) over
the product KP / weight-stationary encoder; the two parts are not separated.  Prints one JSON
line and writes no file: profiles/enctrials_ab.md is written by hand from that line, next to
bench.py's numbers on this change and on the parent (as profiles/kvtrials_ab.md was).

    python tools/enctrials_ab.py [--rounds 5] [--seed 20241223]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "onnx-transformer_amd")):
    sys.path.insert(0, p)


def draw_faults(rng, B, S, n_layers=6):
    """One fault per row in the coordinates of the row's sentence alone."""
    from qtx.fault import random_attn_fault, random_fault
    lins = ("Q", "K", "V", "O", "FFN1", "FFN2")
    kinds = ("INPUT", "WEIGHT", "RANDOM", "INPUT16", "WEIGHT16")
    faults = []
    for b in range(B):
        layer = int(rng.integers(n_layers))
        kind = kinds[(b // 4) % len(kinds)]
        if b % 4 == 3:
            f = random_fault(rng, kind, 1, layer, ("CK", "CV")[(b // 4) % 2], S, bit=7)
        elif b % 4 == 2:
            f = random_attn_fault(rng, "INPUT" if kind == "RANDOM" else kind, 0, layer,
                                  ("QK", "PV")[(b // 4) % 2], 1, S, S, bit=7)
        else:
            f = random_fault(rng, kind, 0, layer, lins[int(rng.integers(len(lins)))], S, bit=7)
        if f.kind == "RANDOM":
            f.value = 3.0e4      # a finite replacement (a drawn one can be inf)
        faults.append(f)
    return faults


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-len", type=int, default=72)
    ap.add_argument("--max-len", type=int, default=72)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241223)
    args = ap.parse_args()
    import torch

    from bench import make_src
    from qtx.decode import (greedy_decode, greedy_decode_enctrials, greedy_decode_fault,
                            greedy_decode_kvfault)
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))
    B, S, L = args.batch, args.src_len, args.max_len
    src, _ = make_src(np.random.default_rng(20241223), B, S)
    mask = (src != 2)[:, None, :]
    faults = draw_faults(np.random.default_rng(args.seed), B, S)

    def alone(b):
        f = faults[b]
        if f.module == 0:
            return greedy_decode_fault(model, src[b:b + 1], mask[b:b + 1], L, 0, fault=f,
                                       return_scores=True)
        return greedy_decode_kvfault(model, src[b:b + 1], mask[b:b + 1], L, 0, fault=f, step=0,
                                     return_scores=True)

    runs = {
        "standalone_32_calls": lambda: [alone(b) for b in range(B)],
        "trials_one_call": lambda: greedy_decode_enctrials(model, src, mask, L, 0, faults),
        "scored_golden": lambda: greedy_decode(model, src, mask, L, 0, return_scores=True),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # warm-up (graphs captured, workspaces at their final size) and the contract on these inputs
    ys, sc = runs["trials_one_call"]()
    rows_equal = True
    for b, (y1, s1) in enumerate(runs["standalone_32_calls"]()):
        rows_equal &= (np.array_equal(ys[b], np.asarray(y1)[0])
                       and np.array_equal(sc.top_ids[b], s1.top_ids[0])
                       and np.array_equal(sc.top_logp[b].view(np.uint32), s1.top_logp[0].view(np.uint32)))
    gy, gs = runs["scored_golden"]()
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "shape": {"B": B, "S": S, "max_len": L}, "rounds": args.rounds, "seed": args.seed,
        "ckv_trials": sum(f.module == 1 for f in faults), "rows_equal_standalone": bool(rows_equal),
        "rows_with_changed_tokens": int((ys != gy).any(1).sum()),
        "rows_with_changed_scores": int((sc.top_logp.view(np.uint32) != gs.top_logp.view(np.uint32)).any((1, 2)).sum()),
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "trials_minus_golden_ms": round(med["trials_one_call"] - med["scored_golden"], 3),
        "ms_per_trial": {"standalone_32_calls": round(med["standalone_32_calls"] / B, 3),
                         "trials_one_call": round(med["trials_one_call"] / B, 3)}}))


if __name__ == "__main__":
    main()
