#!/usr/bin/env python3
"""A/B of the decoder-fault decode in one process at bench.py's shape and inputs (B = 32,
S = 72, max_len = 72), wall time in ms, alternating in rounds so that clock drift hits all
alike:

  (a) greedy_decode_fault(kv_cache=False, return_scores=True): the full-prefix loop, one trial
  (b) greedy_decode_fault(kv_cache=True, return_scores=True) at target_inference_number 1, 36
      and 71: one KV-cached library call per trial
  (c) decode_fault_sweep over --trials INPUT bit flips (uniform steps, linears, elements and
      bits): per trial, the golden decode included
  (d) the same sweep with OUTPUT faults of 3e4 on the last layer's FFN2 at a sentence's last
      position, which change that sentence's token: every trial resumes the decode

Prints one JSON line.

    python tools/dfault_ab.py [--rounds 5] [--trials 64]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-len", type=int, default=72)
    ap.add_argument("--max-len", type=int, default=72)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3, help="cached trials per timed block")
    args = ap.parse_args()
    import torch

    from bench import make_src
    from qtx.decode import decode_fault_sweep, greedy_decode_fault
    from qtx.fault import Fault, random_fault
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))
    B, S, L = args.batch, args.src_len, args.max_len
    src, _ = make_src(np.random.default_rng(20241223), B, S)
    mask = (src != 2)[:, None, :]
    rng = np.random.default_rng(7)
    lins = ("Q", "K", "V", "O", "CQ", "CO", "FFN1", "FFN2")

    def draw(tin):
        return random_fault(rng, "INPUT", 1, int(rng.integers(6)), lins[int(rng.integers(len(lins)))],
                            B * tin, bit=int(rng.integers(8)))

    tins = (1, L // 2, L - 1)
    single = {t: draw(t) for t in tins}
    sweep = []
    for _ in range(args.trials):
        t = int(rng.integers(1, L))
        sweep.append((draw(t), t))

    loud = [(Fault("OUTPUT", 1, 5, "FFN2", row=int(rng.integers(B)) * t + t - 1, col=100, value=3.0e4), t)
            for _, t in sweep]

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, out

    loop = lambda t: greedy_decode_fault(model, src, mask, L, 0, fault=single[t],
                                         target_inference_number=t, return_scores=True)
    cached = lambda t: greedy_decode_fault(model, src, mask, L, 0, fault=single[t],
                                           target_inference_number=t, return_scores=True,
                                           kv_cache=True)
    # warm-up: graphs captured, workspaces at their final size; and the results compared
    same = True
    for t in tins:
        a, b = loop(t), cached(t)
        same &= bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].top_ids, b[1].top_ids)
                     and np.array_equal(a[1].top_logp, b[1].top_logp, equal_nan=True))
    _, stats = decode_fault_sweep(model, src, mask, L, 0, sweep)
    _, stats_d = decode_fault_sweep(model, src, mask, L, 0, loud)
    ta, tb, tc, td = [], {t: [] for t in tins}, [], []
    for _ in range(args.rounds):
        ta.append(timed(lambda: loop(L // 2))[0])
        for t in tins:
            tb[t].append(timed(lambda: cached(t), args.reps)[0])
        tc.append(timed(lambda: decode_fault_sweep(model, src, mask, L, 0, sweep))[0] / len(sweep))
        td.append(timed(lambda: decode_fault_sweep(model, src, mask, L, 0, loud))[0] / len(loud))
    med = statistics.median
    r4 = lambda v: [round(x, 3) for x in v]
    print(json.dumps({
        "shape": {"B": B, "S": S, "max_len": L}, "rounds": args.rounds,
        "loop_ms": r4(ta), "loop_median_ms": round(med(ta), 3),
        "cached_ms": {str(t): r4(v) for t, v in tb.items()},
        "cached_median_ms": {str(t): round(med(v), 3) for t, v in tb.items()},
        "sweep_ms_per_trial": r4(tc), "sweep_median_ms_per_trial": round(med(tc), 3),
        "sweep_trials": len(sweep), "sweep_resumed": stats.n_resumed,
        "sweep_skipped": stats.n_skipped,
        "loud_sweep_ms_per_trial": r4(td), "loud_sweep_median_ms_per_trial": round(med(td), 3),
        "loud_sweep_resumed": stats_d.n_resumed, "loud_sweep_skipped": stats_d.n_skipped,
        "results_equal": same}))


if __name__ == "__main__":
    main()
