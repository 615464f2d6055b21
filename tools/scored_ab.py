#!/usr/bin/env python3
"""A/B of the plain and the scored greedy decode in one process, at bench.py's shape and
inputs (B = 32, S = 72, max_len = 72): wall time per decode, plain | scored alternating in
rounds so that clock drift hits both alike.  Prints one JSON line.

    python tools/scored_ab.py [--rounds 7] [--reps 20]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="decodes per timed block")
    args = ap.parse_args()
    import torch

    from bench import make_src
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))
    B, S, L = args.batch, args.src_len, args.max_len
    src, _ = make_src(np.random.default_rng(20241223), B, S)
    srcd = torch.from_numpy(src).cuda()
    maskd = (srcd != 2).to(torch.uint8)
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")

    def plain():
        model.greedy(srcd, maskd, max_len=L, start=0, out=ids)

    def scored():
        return model.greedy(srcd, maskd, max_len=L, start=0, out=ids, scores=True)

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3

    # both graphs captured and the workspace at its final size before anything is timed
    scored()
    plain()
    p_ids = ids.clone()
    _, top_ids, _ = scored()
    torch.cuda.synchronize()
    same = bool((p_ids == ids).all() and (top_ids[..., 0] == ids[:, 1:]).all())
    block(plain), block(scored)
    tp, ts = [], []
    for _ in range(args.rounds):
        tp.append(block(plain))
        ts.append(block(scored))
    mp, ms = statistics.median(tp), statistics.median(ts)
    print(json.dumps({"shape": {"B": B, "S": S, "max_len": L}, "reps": args.reps,
                      "plain_ms": [round(t, 4) for t in tp], "scored_ms": [round(t, 4) for t in ts],
                      "plain_median_ms": round(mp, 4), "scored_median_ms": round(ms, 4),
                      "scored_over_plain": round(ms / mp, 4), "ids_equal": same}))


if __name__ == "__main__":
    main()
