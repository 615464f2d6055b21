#!/usr/bin/env python3
"""Wall time of one B = 32 greedy decode (bench.py's cfg2 shape: S = 72, max_len = 72) of the
six-layer d_ff = 2048 model with 4, 8 and 16 heads, random weights, in one process: two warm-up
decodes per model (graph capture, workspace), then --rounds rounds that visit the three models
in turn, --reps decodes each, every decode ending in a device synchronise.  Prints one JSON line
with each model's median and spread in ms.

    python tools/heads_decode_time.py [--rounds 3] [--reps 5]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "onnx-transformer_amd")):
    sys.path.insert(0, p)
B, S, L = 32, 72, 72


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from qtx.decode import greedy_decode
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict
    rng = np.random.default_rng(3)
    src = torch.from_numpy(rng.integers(4, 5000, (B, S))).cuda()
    mask = torch.ones((B, 1, S), dtype=torch.bool, device="cuda")
    models, times = {}, {}
    for H in (4, 8, 16):
        cfg = dataclasses.replace(ModelConfig(), n_heads=H, max_len=128)
        models[H] = QtxModel(synthetic_state_dict(7, cfg, ln_random=True), cfg)
        times[H] = []
        for _ in range(2):
            greedy_decode(models[H], src, mask, L, 0)
    for _ in range(a.rounds):
        for H, gm in models.items():
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                greedy_decode(gm, src, mask, L, 0)
                torch.cuda.synchronize()
                times[H].append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({f"heads_{H}": {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                                     "max_ms": round(max(t), 3), "n": len(t)} for H, t in times.items()}))


if __name__ == "__main__":
    main()
