#!/usr/bin/env python3
"""Wall time of qtx_greedy_decode_kvfault in one process at bench.py's shape and inputs (B = 32,
S = 72, max_len = 72), in ms as the caller sees it, alternating in rounds so that clock drift
hits all alike:

  (a) greedy_decode(return_scores=True): the scored golden decode
  (b) greedy_decode_fault(kv_cache=True, return_scores=True) at the same step: the campaign
      semantics' KV-cached call (qtx_greedy_decode_dfault)
  (c) greedy_decode_kvfault(fault=..., return_scores=True): a step fault (INPUT on a V
      projection) at --step
  (d) greedy_decode_kvfault(fault=...) on an attention target (WEIGHT on PV)
  (e) greedy_decode_kvfault(upset=..., return_scores=True): a self-V code upset at --step

Prints one JSON line.

    python tools/kvfault_ab.py [--rounds 5] [--step 36]
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
    ap.add_argument("--step", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed block")
    args = ap.parse_args()
    import torch

    from bench import make_src
    from qtx.decode import greedy_decode, greedy_decode_fault, greedy_decode_kvfault
    from qtx.fault import CacheUpset, Fault
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))
    B, S, L, i = args.batch, args.src_len, args.max_len, args.step
    src, _ = make_src(np.random.default_rng(20241223), B, S)
    mask = (src != 2)[:, None, :]
    f_lin = Fault("INPUT", 1, 2, "V", row=5, col=50, bit=7)
    f_camp = Fault("INPUT", 1, 2, "V", row=5 * (i + 1) + i, col=50, bit=7)
    f_attn = Fault("WEIGHT", 1, 2, "PV", row=5 * (i + 1) + i // 2, col=2 * 64 + 7, bit=7)
    upset = CacheUpset("self_v", 2, row=5 * L + i // 2, col=70, bit=7)
    runs = {
        "scored_golden": lambda: greedy_decode(model, src, mask, L, 0, return_scores=True),
        "dfault_cached": lambda: greedy_decode_fault(model, src, mask, L, 0, fault=f_camp,
                                                     target_inference_number=i + 1,
                                                     return_scores=True, kv_cache=True),
        "kvfault_linear": lambda: greedy_decode_kvfault(model, src, mask, L, 0, fault=f_lin, step=i,
                                                        return_scores=True),
        "kvfault_attention": lambda: greedy_decode_kvfault(model, src, mask, L, 0, fault=f_attn,
                                                           step=i, return_scores=True),
        "kvfault_upset": lambda: greedy_decode_kvfault(model, src, mask, L, 0, upset=upset, step=i,
                                                       return_scores=True),
    }

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    for fn in runs.values():       # warm-up: graphs captured, workspaces at their final size
        fn()
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn, args.reps))
    print(json.dumps({
        "shape": {"B": B, "S": S, "max_len": L}, "step": i, "rounds": args.rounds,
        "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
