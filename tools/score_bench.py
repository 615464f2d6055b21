"""Teacher-forced target scoring against the composed path of the older entry points, at cfg2's
shape (B = 32, S = 72, L = 72, the full-size synthetic model) — profiles/score_bench.md,
DESIGN.md (target scoring).  Not wired into bench.py.

    python tools/score_bench.py time [--rounds 5] [--window 1.0]
        alternating rounds, device events around enough repetitions for `window` seconds each:
          (a) score      QtxModel.score on the model's own greedy ids (one library call)
          (b) composed   embed + encode + embed + decode + generator(want_logp=True) + a torch
                         gather, topk(2) and a rank count on the [B*T, V] log-probabilities
          (c) greedy     greedy(scores=True) at the same shape, for scale
        then 8 decoder-fault trials in one call against 8 stand-alone one-fault calls, and the
        generator chunk: qtx_score_rows on the same B*T rows with workspace for 64 / 256 / 928 /
        all rows (the model-level call's chunk at this shape).  Medians and the spread (max - min over the rounds).
    python tools/score_bench.py trace [--calls 20]
        (a) alone, for `rocprofv3 --kernel-trace --stats -- python tools/score_bench.py trace`.
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "onnx-transformer_amd")]
B, S, L = 32, 72, 72


def make_src(rng):
    src = np.full((B, S), 2, np.int64)
    for b in range(B):
        n = S if b % 4 == 0 else int(rng.integers(S // 2, S))
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
    return src


def setup(greedy=True):
    import torch     # (first: its HIP runtime is the one libqtx must find loaded)
    from qtx.model import QtxModel, to_u8_mask
    from qtx.weights import synthetic_state_dict
    model = QtxModel(synthetic_state_dict(20241223, ln_random=True))
    src = make_src(np.random.default_rng(11))
    s = torch.from_numpy(src).to(model.device)
    m = to_u8_mask((src != 2)[:, None, :], model.device).reshape(B, S)
    if greedy:
        tgt = model.greedy(s, m, max_len=L).clone()
    else:            # the trace: seeded ids, so that no decode's kernels sit among the call's
        ids = np.random.default_rng(12).integers(4, model.cfg.tgt_vocab, (B, L))
        ids[:, 0] = 0
        tgt = torch.from_numpy(ids).to(model.device)
    return torch, model, s, m, tgt


def per_call_ms(torch, fn, window):
    """ms per call: device events around enough calls for `window` seconds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, math.ceil(window * 1e3 / max(e0.elapsed_time(e1) / 3, 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def rounds_of(torch, cases, rounds, window):
    for fn in cases.values():          # warm-up: code objects, workspace growth, graph capture
        for _ in range(3):
            fn()
    times = {k: [] for k in cases}
    reps = {}
    for _ in range(rounds):            # alternating
        for k, fn in cases.items():
            t, reps[k] = per_call_ms(torch, fn, window)
            times[k].append(t)
    for k, v in times.items():
        print(f"{k:34s} median {statistics.median(v):9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}  "
              f"spread {max(v) - min(v):7.3f}  ({len(v)} rounds x {reps[k]} calls)", flush=True)
    return {k: statistics.median(v) for k, v in times.items()}


def time_(args):
    torch, model, s, m, tgt = setup()
    from qtx import _lib
    from qtx.fault import Fault
    T, V, dev = L - 1, model.cfg.tgt_vocab, model.device
    M = B * T
    tm = torch.tril(torch.ones((T, T), dtype=torch.uint8, device=dev))
    labels = tgt[:, 1:].reshape(M, 1)

    def composed():
        memory = model.encode(model.embed(s, "src"), m)
        out = model.decode(model.embed(tgt[:, :T].contiguous(), "tgt"), memory, m, tm)
        logp, _ = model.generator(out.reshape(M, 512), want_logp=True)
        tok = logp.gather(1, labels)
        rank = (logp > tok).sum(1)
        top = torch.topk(logp, 2, dim=1)
        return tok, rank, top

    print(f"shape B={B} S={S} L={L}: M = {M} rows, V = {V}", flush=True)
    rounds_of(torch, {
        "(a) score": lambda: model.score(s, m, tgt, pad=-1),
        "(a') score, no top 2": lambda: model.score(s, m, tgt, pad=-1, return_top2=False),
        "(b) composed": composed,
        "(c) greedy scored": lambda: model.greedy(s, m, max_len=L, scores=True),
    }, args.rounds, args.window)
    rng = np.random.default_rng(5)
    faults = [Fault("INPUT", 1, int(rng.integers(6)), "FFN1", row=int(rng.integers(M)),
                    col=int(rng.integers(512)), bit=6) for _ in range(8)]
    rounds_of(torch, {
        "8 fault trials, one call": lambda: model.score(s, m, tgt, pad=-1, faults=faults),
        "8 stand-alone one-fault calls": lambda: [model.score(s, m, tgt, pad=-1, faults=[f]) for f in faults],
    }, max(3, args.rounds - 2), args.window)
    # the generator chunk, through the per-op entry (its chunk follows the workspace given)
    P = lambda t: C.c_void_p(t.data_ptr())
    x = torch.randn((M, 512), dtype=torch.float32, device=dev)
    y = labels.reshape(M).contiguous()
    tok = torch.empty((M,), dtype=torch.float32, device=dev)
    rank = torch.empty((M,), dtype=torch.int32, device=dev)
    ti = torch.empty((M, 2), dtype=torch.int64, device=dev)
    tv = torch.empty((M, 2), dtype=torch.float32, device=dev)
    cases = {}
    for rows in (64, 256, 928, (M + 15) & ~15):
        ws = torch.empty(rows * V * 4, dtype=torch.uint8, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        cases[f"score_rows chunk {min(rows, M)}"] = lambda ws=ws: _lib.call(
            "qtx_score_rows", model.handle, P(x), M, P(y), P(tok), P(rank), P(ti), P(tv), P(ws),
            ws.numel(), st)
    rounds_of(torch, cases, max(3, args.rounds - 2), args.window)


def trace(args):
    torch, model, s, m, tgt = setup(greedy=False)
    for _ in range(args.calls):
        model.score(s, m, tgt, pad=-1)
    torch.cuda.synchronize()
    print(f"{args.calls} score calls at B={B} S={S} L={L}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "trace"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    time_(a) if a.what == "time" else trace(a)
