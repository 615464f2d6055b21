#!/usr/bin/env python3
"""Wall time of the plain and the scored greedy decode and of beam 4 on models whose d_ff is
neither 512 nor 2048, for two builds of the library in one session: this tree's and another
one's (the parent commit's libqtx.so, --other: it decodes these models with the unfused step).
The 6+6-layer model with random weights at d_ff = 1024 and 768, bench.py's 32 sentences, S = 72,
max_len = 72.  Each leg is a child process on one library (QTX_LIB_PATH): two warm-up decodes
per (d_ff, kind) (graph capture, workspace), then --reps timed ones, each ending in a device
synchronise.  The legs alternate, other / this, for --rounds rounds.  Prints one JSON line per
leg and a last one with the medians, each side's spread and whether both builds gave the same
ids (profiles/dff_fused_ab.md).

    python tools/dff_ab.py --other /path/to/parent/libqtx.so [--rounds 2] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/dff_ab.py --leg   (kernel times)
"""
import argparse
import ctypes
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
S, L = 72, 72
D_FFS = (1024, 768)
KINDS = ("plain", "scored", "beam4")


def leg(reps, batch):
    """One library (whatever QTX_LIB_PATH names): {"<d_ff>/<kind>": {ms: [...], ids_crc}}."""
    import torch

    from bench import make_src
    from qtx import _lib
    if os.environ.get("QTX_LIB_PATH"):      # an older build: bind only the entry points it has
        old = ctypes.CDLL(os.environ["QTX_LIB_PATH"])
        for name in [n for n in dir(_lib) if n.startswith("SIGNATURES")]:
            setattr(_lib, name, {k: v for k, v in getattr(_lib, name).items() if hasattr(old, k)})
    from qtx.decode import beam_decode, greedy_decode
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict

    src, _ = make_src(np.random.default_rng(20241223), batch, S)
    mask = (src != 2)[:, None, :]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for d_ff in D_FFS:
        cfg = ModelConfig(d_ff=d_ff)
        model = QtxModel(synthetic_state_dict(20241223, cfg), cfg)
        runs = {"plain": lambda: greedy_decode(model, src, mask, L, 0),
                "scored": lambda: greedy_decode(model, src, mask, L, 0, return_scores=True)[0],
                "beam4": lambda: beam_decode(model, src, mask, L, 0, beam_size=4, early_exit=False).ids}
        for kind in KINDS:
            runs[kind]()
            ids = runs[kind]()
            out[f"{d_ff}/{kind}"] = {"ms": [round(timed(runs[kind]), 3) for _ in range(reps)],
                                     "ids_crc": zlib.crc32(np.ascontiguousarray(ids).tobytes())}
        del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the other build's libqtx.so (the parent commit's)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(args.reps),
                                "--batch", str(args.batch)],
                               env=dict(os.environ, QTX_LIB_PATH=path), capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"leg {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            got[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps({"round": r, "lib": name, "result": got[name][-1]}), flush=True)
    summary = {}
    for key in [f"{d}/{k}" for d in D_FFS for k in KINDS]:
        row = {}
        for name in libs:
            ms = [x for res in got[name] for x in res[key]["ms"]]
            row[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": min(ms), "max_ms": max(ms)}
        row["ids_equal"] = len({res[key]["ids_crc"] for name in libs for res in got[name]}) == 1
        row["other_over_this"] = round(row["other"]["median_ms"] / row["this"]["median_ms"], 3)
        summary[key] = row
    print(json.dumps({"batch": args.batch, "rounds": args.rounds, "reps": args.reps, "median": summary}))


if __name__ == "__main__":
    main()
