#!/usr/bin/env python3
"""Every model-level driver of the C-ABI once, eagerly (QTX_NO_GRAPH=1: each step's kernels
are launched, not replayed from a graph), on a small model (two layers, d_ff 512, the fused
step's smallest config) at B = 2, S = 5, max_len = 6: greedy plain and scored, the unfused
step (QTX_UNFUSED=1), dfault and dfault_resume, kvfault with a linear fault, an attention
fault, a CK fault and an upset, beam with beam = 2, score_targets with tgt_per_src = 2 and
with one decoder fault at tgt_per_src = 1.  Prints one JSON line: a digest of every driver's
outputs.

Under a kernel trace the run gives the ordered list of launches of all drivers, which a change
of host code alone must leave as it is:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_seq.py
    python tools/launch_seq.py --compare A_kernel_trace.csv B_kernel_trace.csv

--compare reads two such traces and compares (kernel name, grid, workgroup size) launch by
launch, in start order; exit status 1 and the first difference when they differ.
"""
import argparse
import csv
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "onnx-transformer_amd")):
    sys.path.insert(0, p)


def launches(path):
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dims = [k for k in rows[0] if k.startswith(("Grid_Size", "Workgroup_Size"))] if rows else []
    return [(r["Kernel_Name"],) + tuple(int(r[k]) for k in dims) for r in rows]


def compare(a, b):
    la, lb = launches(a), launches(b)
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"launch {i} differs:\n  {a}: {x}\n  {b}: {y}")
            return 1
    if len(la) != len(lb):
        print(f"{len(la)} launches in {a}, {len(lb)} in {b}")
        return 1
    print(json.dumps({"launches": len(la), "distinct_kernels": len({x[0] for x in la}),
                      "identical": True}))
    return 0


def digest(out):
    import torch
    h = hashlib.sha256()
    for t in out if isinstance(out, (tuple, list)) else (out,):
        if isinstance(t, torch.Tensor):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        elif t is not None:
            h.update(repr(t if not hasattr(t, "tobytes") else t.tobytes()).encode())
    return h.hexdigest()[:16]


def run():
    os.environ["QTX_NO_GRAPH"] = "1"
    import numpy as np
    import torch

    from qtx import _lib
    from qtx.fault import CacheUpset, Fault
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict

    cfg = ModelConfig(src_vocab=97, tgt_vocab=89, n_layers=2, d_ff=512, max_len=64)
    model = QtxModel(synthetic_state_dict(20241223, cfg), cfg)
    B, S, L = 2, 5, 6
    rng = np.random.default_rng(7)
    dev = model.device
    src = torch.from_numpy(rng.integers(3, cfg.src_vocab, (B, S))).to(dev)
    mask = torch.ones((B, S), dtype=torch.uint8, device=dev)
    mask[1, S - 1] = 0
    tgt = lambda rows: torch.from_numpy(rng.integers(3, cfg.tgt_vocab, (rows, L + 1))).to(dev)
    f_lin = Fault("INPUT", 1, 1, "V", row=1, col=50, bit=6)
    f_pass = Fault("INPUT", 1, 1, "V", row=1 * 3 + 2, col=50, bit=6)     # step 2: T = 3 rows a sentence
    f_attn = Fault("WEIGHT", 1, 0, "PV", row=1 * 3 + 1, col=2 * 64 + 7, bit=6)
    f_ck = Fault("INPUT", 1, 1, "CK", row=S + 2, col=9, bit=6)
    upset = CacheUpset("self_v", 1, row=1 * L + 1, col=70, bit=6)
    out = {}
    out["greedy"] = digest(model.greedy(src, mask, L))
    out["greedy_scored"] = digest(model.greedy(src, mask, L, scores=True))
    os.environ["QTX_UNFUSED"] = "1"
    _lib.reload_knobs()
    out["greedy_unfused"] = digest(model.greedy(src, mask, L))
    del os.environ["QTX_UNFUSED"]
    _lib.reload_knobs()
    ws = model.dfault_workspace(B, S, L)
    out["dfault"] = digest(model.greedy_dfault(src, mask, f_pass, 2, L, scores=True, ws=ws))
    out["dfault_resume"] = digest(model.greedy_dfault_resume(ws, B, S, f_pass, 2, L))
    out["kvfault_linear"] = digest(model.greedy_kvfault(src, mask, 2, fault=f_lin, max_len=L, scores=True))
    out["kvfault_attention"] = digest(model.greedy_kvfault(src, mask, 2, fault=f_attn, max_len=L, scores=True))
    out["kvfault_ck"] = digest(model.greedy_kvfault(src, mask, 0, fault=f_ck, max_len=L, scores=True))
    out["kvfault_upset"] = digest(model.greedy_kvfault(src, mask, 2, upset=upset, max_len=L, scores=True))
    out["beam"] = digest(model.beam(src, mask, L, beam_size=2, early_exit=False))
    out["score_k2"] = digest(model.score(src, mask, tgt(2 * B), tgt_per_src=2))
    f_dec = Fault("INPUT", 1, 0, "FFN1", row=L + 1, col=11, bit=6)
    out["score_fault"] = digest(model.score(src, mask, tgt(B), faults=[f_dec]))
    torch.cuda.synchronize()
    model.check()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="CSV")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run())


if __name__ == "__main__":
    main()
