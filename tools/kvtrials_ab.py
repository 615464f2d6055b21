#!/usr/bin/env python3
"""Wall time per kvfault trial in one process at bench.py's shape and inputs (S = 72,
max_len = 72, the cfg2 model): 32 trials, one per sentence of bench.py's batch, their steps drawn
uniformly over the decode's steps from a fixed seed, the kinds cycling through a linear step
fault, an attention step fault and a cache upset.  In ms as the caller sees it, alternating in
rounds so that clock drift hits all alike:

  (a) 32 stand-alone greedy_decode_kvfault(return_scores=True) calls, one sentence each (B = 1)
  (b) one greedy_decode_kvfault_trials call on the 32 rows (qtx_greedy_decode_kvtrials)
  (c) greedy_decode(return_scores=True) on the 32 rows: the scored golden decode

Before timing, every row of (b) is compared with its call of (a), bit for bit.  Prints one JSON
line: the legs' ms per round, the medians, and ms per trial for (a) and (b).

    python tools/kvtrials_ab.py [--rounds 5] [--seed 20241223]
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


def draw_trials(rng, B, S, L, n_layers=6):
    """One trial per row in the coordinates of the row's sentence alone."""
    from qtx.fault import CacheUpset, Fault, random_fault
    lins = ("Q", "K", "V", "O", "CQ", "CO", "FFN1", "FFN2")
    trials = []
    for b in range(B):
        step = int(rng.integers(0, L - 1))
        layer = int(rng.integers(n_layers))
        if b % 3 == 0:
            kind = ("INPUT", "WEIGHT", "RANDOM", "INPUT16")[(b // 3) % 4]
            f = random_fault(rng, kind, 1, layer, lins[int(rng.integers(len(lins)))], 1, bit=7)
            if kind == "RANDOM":
                f.value = 3.0e4      # a finite replacement (a drawn one can be inf)
        elif b % 3 == 1:
            j = int(rng.integers(step + 1))
            f = Fault("WEIGHT", 1, layer, "PV", row=j, col=int(rng.integers(512)), bit=7)
        elif step >= 1:
            f = CacheUpset("self_v", layer, row=int(rng.integers(step)), col=int(rng.integers(512)), bit=7)
        else:
            f = CacheUpset("cross_v", layer, row=int(rng.integers(S)), col=int(rng.integers(512)), bit=7)
        trials.append((f, step))
    return trials


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
    from qtx.decode import greedy_decode, greedy_decode_kvfault, greedy_decode_kvfault_trials
    from qtx.fault import Fault
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))
    B, S, L = args.batch, args.src_len, args.max_len
    src, _ = make_src(np.random.default_rng(20241223), B, S)
    mask = (src != 2)[:, None, :]
    trials = draw_trials(np.random.default_rng(args.seed), B, S, L)

    def alone(b):
        what, step = trials[b]
        kw = {"fault": what} if isinstance(what, Fault) else {"upset": what}
        return greedy_decode_kvfault(model, src[b:b + 1], mask[b:b + 1], L, 0, step=step,
                                     return_scores=True, **kw)

    runs = {
        "standalone_32_calls": lambda: [alone(b) for b in range(B)],
        "trials_one_call": lambda: greedy_decode_kvfault_trials(model, src, mask, L, 0, trials),
        "scored_golden": lambda: greedy_decode(model, src, mask, L, 0, return_scores=True),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # warm-up (graphs captured, workspaces at their final size) and the contract on these inputs
    ys, sc, recs = runs["trials_one_call"]()
    rows_equal = True
    for b, (y1, s1) in enumerate(runs["standalone_32_calls"]()):
        r1 = s1.fault_step
        rows_equal &= (np.array_equal(ys[b], y1[0]) and np.array_equal(sc.top_ids[b], s1.top_ids[0])
                       and np.array_equal(sc.top_logp[b].view(np.uint32), s1.top_logp[0].view(np.uint32))
                       and np.array_equal(recs[b].faulty_logp.view(np.uint32),
                                          r1.faulty_logp[0].view(np.uint32))
                       and np.array_equal(recs[b].golden_ids, r1.golden_ids[0]))
    gy, _ = runs["scored_golden"]()
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({
        "shape": {"B": B, "S": S, "max_len": L}, "rounds": args.rounds, "seed": args.seed,
        "distinct_steps": len({s for _, s in trials}), "rows_equal_standalone": bool(rows_equal),
        "rows_with_changed_tokens": int((ys != gy).any(1).sum()),
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "ms_per_trial": {"standalone_32_calls": round(med["standalone_32_calls"] / B, 3),
                         "trials_one_call": round(med["trials_one_call"] / B, 3)}}))


if __name__ == "__main__":
    main()
