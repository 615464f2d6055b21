#!/usr/bin/env python3
"""Attention past 128 keys, for two builds of the library in one session: this tree's and
another one's (the parent commit's libqtx.so, --other).  Times one qtx_attention_i8 launch at
B = 32, H = 8 for the shapes of SHAPES (encoder-shaped with a key mask, decoder-shaped with a
causal mask, cross-shaped, one query row), qtx_encoder_forward at B = 32, S = 512 and
qtx_score_targets at S = 72, L = 512 on the cfg2 model.  Each leg is a child process on one
library (QTX_LIB_PATH): per line 3 warm-up calls, then --reps windows of --iters calls between
device events.  The legs alternate, other / this, for --rounds rounds, so that clock drift hits
both alike.  Prints one JSON line per leg and a markdown table of the medians with each line's
run-to-run spread (min .. max over all its windows) and whether both builds wrote the same bits.

    python tools/attn_long_ab.py --other /path/to/parent/libqtx.so [--rounds 3] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "onnx-transformer_amd")):
    sys.path.insert(0, p)

B, H = 32, 8
# (name, Sq, Sk, mask form, dec)
SHAPES = [(f"enc {S}x{S} key mask", S, S, "key", 0) for S in (130, 256, 512)] + \
         [(f"dec {S}x{S} causal", S, S, "causal", 1) for S in (130, 256, 512)] + \
         [("cross 72x512 key mask", 72, 512, "key", 1), ("one row 1x512 key mask", 1, 512, "key", 1)]


def leg(reps, iters):
    """One library (whatever QTX_LIB_PATH names): {line: {"us": [...], "crc": ...}}."""
    import torch

    from qtx import _lib
    from qtx.decode import score_targets
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict

    raw = C.CDLL(os.environ.get("QTX_LIB_PATH") or _lib._build.LIB)
    for n in [n for n in _lib.SIGNATURES if not hasattr(raw, n)]:
        del _lib.SIGNATURES[n]               # an entry the other build predates: not bound
    L = _lib.lib(build=False)
    P = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    S0 = C.c_void_p(0)

    def windows(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1) / n * 1e3, 2))
        return out

    crc = lambda t: zlib.crc32(t.cpu().numpy().tobytes())   # noqa: E731
    res = {}
    rng = np.random.default_rng(20241223)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    for name, Sq, Sk, form, dec in SHAPES:
        q = T(rng.integers(-127, 128, (B, Sq, 512)).astype(np.int8))
        k, v = (T(rng.integers(-127, 128, (B, Sk, 512)).astype(np.int8)) for _ in range(2))
        sq, sk, sv = (T(rng.uniform(0.002, 0.03, (B, n)).astype(np.float32)) for n in (Sq, Sk, Sk))
        if form == "key":
            km = np.ones((B, Sk), np.uint8)
            for b in range(B):
                km[b, Sk - (b * Sk) // (2 * B):] = b % 4 == 0     # three sentences in four padded
            mask, m_bs, m_is = T(km), Sk, 0
        else:
            mask, m_bs, m_is = T(np.tril(np.ones((Sq, Sk), np.uint8), k=Sk - Sq)), 0, Sk
        ctx = torch.empty((B, Sq, 512), device="cuda")
        fn = lambda: L.qtx_attention_i8(P(q), P(sq), P(k), P(sk), P(v), P(sv), P(mask), m_bs, m_is,   # noqa: E731
                                        B, H, Sq, Sk, P(ctx), dec, S0)
        res[name] = {"us": windows(fn, iters), "crc": crc(ctx)}

    model = QtxModel(synthetic_state_dict(20241223))
    x = torch.from_numpy(rng.standard_normal((B, 512, 512)).astype(np.float32)).cuda()
    mk = torch.ones((B, 512), dtype=torch.uint8, device="cuda")
    res["qtx_encoder_forward 32x512"] = {"us": windows(lambda: model.encode(x, mk), 3),
                                         "crc": crc(model.encode(x, mk))}
    src = rng.integers(4, 5337, (B, 72))
    tgt = rng.integers(4, 4444, (B, 512))
    srcd, tgtd = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    smask = torch.ones((B, 1, 72), dtype=torch.bool, device="cuda")
    score = lambda: score_targets(model, srcd, smask, tgtd, pad=-1)   # noqa: E731
    res["qtx_score_targets S=72 L=512"] = {"us": windows(score, 3), "crc": crc(score().tok_logp)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the other build's libqtx.so (the parent commit's)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--leg", action="store_true", help="(child) time the library in QTX_LIB_PATH")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.reps, args.iters)), flush=True)
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
                                "--iters", str(args.iters)], env=env, capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"leg {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            got[name].append(res)
            print(json.dumps({"round": r, "lib": name, "result": res}), flush=True)
    print(f"\n| line | other us (min .. max) | this us (min .. max) | other / this | same bits |\n|---|---|---|---|---|")
    for line in got["this"][0]:
        cell, med = {}, {}
        for name in libs:
            us = [x for res in got[name] for x in res[line]["us"]]
            med[name] = statistics.median(us)
            cell[name] = f"{med[name]:.1f} ({min(us):.1f} .. {max(us):.1f})"
        same = len({res[line]["crc"] for name in libs for res in got[name]}) == 1
        print(f"| {line} | {cell['other']} | {cell['this']} | {med['other'] / med['this']:.2f} | {'yes' if same else 'NO'} |")


if __name__ == "__main__":
    main()
