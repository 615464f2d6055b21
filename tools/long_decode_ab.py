#!/usr/bin/env python3
"""Wall time of the plain greedy decode at and past 128 keys, for two builds of the library in
one session: this tree's and another one's (the parent commit's libqtx.so, --other), the cfg2
model and bench.py's 32 sentences.  Shapes (S, max_len): (72, 72), (72, 140), (72, 256),
(72, 512) and (160, 72).  Each leg is a child process on one library (QTX_LIB_PATH): the first
call of every shape timed on its own (it captures and instantiates the step graphs), one more
warm-up, then --reps timed decodes.  The legs alternate, other / this, for --rounds rounds, so
that clock drift hits both alike.  Prints one JSON line per leg and a last one with the
medians: ms per decode, ms per step, the first call, and whether both builds decoded the
same ids.

    python tools/long_decode_ab.py --other /path/to/parent/libqtx.so [--rounds 3] [--reps 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "onnx-transformer_amd")):
    sys.path.insert(0, p)

SHAPES = [(72, 72), (72, 140), (72, 256), (72, 512), (160, 72)]


def leg(reps, batch):
    """One library (whatever QTX_LIB_PATH names): {"S,max_len": {first_ms, ms: [...]}}."""
    import torch

    from bench import make_src
    from qtx.decode import greedy_decode
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    model = QtxModel(synthetic_state_dict(20241223))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for S, L in SHAPES:
        src, _ = make_src(np.random.default_rng(20241223), batch, S)
        mask = (src != 2)[:, None, :]
        run = lambda: greedy_decode(model, src, mask, L, 0)
        first = timed(run)
        crc = zlib.crc32(np.ascontiguousarray(run()).tobytes())     # the ids: equal across builds
        out[f"{S},{L}"] = {"first_ms": round(first, 3), "ms": [round(timed(run), 3) for _ in range(reps)],
                           "ids_crc": crc}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the other build's libqtx.so (the parent commit's)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", action="store_true", help="(child) time the library in QTX_LIB_PATH")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.reps, args.batch)), flush=True)
        return
    if not args.other:
        ap.error("--other is required")
    libs = {"other": os.path.abspath(args.other),
            "this": os.path.join(REPO, "onnx-transformer_amd", "qtx", "libqtx.so")}
    got = {k: [] for k in libs}
    for r in range(args.rounds):
        for name, path in libs.items():
            env = dict(os.environ, QTX_LIB_PATH=path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(args.reps),
                                "--batch", str(args.batch)], env=env, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"leg {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            got[name].append(res)
            print(json.dumps({"round": r, "lib": name, "result": res}), flush=True)
    summary = {}
    for S, L in SHAPES:
        key = f"{S},{L}"
        row = {}
        for name in libs:
            ms = statistics.median(x for res in got[name] for x in res[key]["ms"])
            row[name] = {"ms_per_decode": round(ms, 3), "ms_per_step": round(ms / (L - 1), 4),
                         "first_ms": round(statistics.median(res[key]["first_ms"] for res in got[name]), 3)}
        row["ids_equal"] = len({res[key]["ids_crc"] for name in libs for res in got[name]}) == 1
        row["other_over_this"] = round(row["other"]["ms_per_decode"] / row["this"]["ms_per_decode"], 3)
        summary[key] = row
    print(json.dumps({"batch": args.batch, "rounds": args.rounds, "reps": args.reps, "median": summary}))


if __name__ == "__main__":
    main()
