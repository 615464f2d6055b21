"""Beam decode against the greedy decode at the same row count, and the in-graph cost of the
two beam kernels (profiles/beam_ab.md).  Not wired into bench.py.

    python tools/beam_ab.py decode [--lib PATH] [--rounds 7]
        cfg2's shape (S = 72, max_len = 72, the default model): alternating rounds of
          beam     B = 32, beam = 4, early_exit off   (128 rows, beam tail)
          greedy   B = 128                            (128 rows, argmax tail)
          greedy   B = 32
        and the medians (ms per decode, us per step).  --lib: another build of libqtx.so (the
        parent commit's: the greedy lines then measure that build; no beam line).
    python tools/beam_ab.py kernels
        k_beam_select and k_beam_reorder alone: 50 launches each in one captured graph at
        cfg2's shape (128 rows, the model's vocabulary, 6 layers), us per launch, at
        positions 8 / 36 / 70 and with an identity / a shuffled parent vector.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "onnx-transformer_amd")]


def make_src(rng, B, S):
    src = np.full((B, S), 2, np.int64)
    for b in range(B):
        n = S if b % 4 == 0 else int(rng.integers(S // 2, S))
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
    return src


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def decode(args):
    import torch     # (first: its HIP runtime is the one libqtx must find loaded)
    if args.lib:     # an older build: bind only the entry points it has
        os.environ["QTX_LIB_PATH"] = args.lib
        from qtx import _lib
        old = C.CDLL(args.lib)
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(old, k)}
    from qtx.model import QtxModel, to_u8_mask
    from qtx.weights import synthetic_state_dict
    model = QtxModel(synthetic_state_dict(20241223))
    S = L = 72
    rng = np.random.default_rng(11)
    dev = model.device
    cases = {}
    for B in (32, 128):
        src = make_src(rng, B, S)
        s = torch.from_numpy(src).to(dev)
        m = to_u8_mask((src != 2)[:, None, :], dev).reshape(B, S)
        cases[f"greedy B={B}"] = lambda s=s, m=m: model.greedy(s, m, max_len=L)
        if B == 32 and not args.lib and not args.no_beam:
            cases["beam B=32 beam=4"] = lambda s=s, m=m: model.beam(s, m, max_len=L, beam_size=4,
                                                                   early_exit=False)
    for fn in cases.values():          # warm-up: graph capture, workspace growth
        for _ in range(3):
            fn()
    times = {k: [] for k in cases}
    for _ in range(args.rounds):       # alternating rounds
        for k, fn in cases.items():
            times[k].append(timed(fn, torch))
    for k, v in times.items():
        med = statistics.median(v)
        print(f"{k:20s} median {med:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
              f"({med * 1e3 / (L - 1):7.1f} us/step, {len(v)} rounds)", flush=True)


def kernels(args):
    import torch
    from qtx import _lib
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict
    model = QtxModel(synthetic_state_dict(20241223))
    lib = _lib.lib(build=False)
    V, B, K, ML, NL = model.cfg.tgt_vocab, 32, 4, 72, 6
    R = B * K
    P = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    logits = T((rng.standard_normal((R, V)) * 2).astype(np.float32))
    krow, vrow = ML * 512, ((ML + 3) // 4) * 2048
    kc = torch.zeros((NL, R, krow), dtype=torch.int8, device="cuda")
    vc = torch.zeros((NL, R, vrow), dtype=torch.int8, device="cuda")
    skc = torch.zeros((NL, R, ML), dtype=torch.float32, device="cuda")
    svc = torch.zeros((NL, R, ML), dtype=torch.float32, device="cuda")
    bp = torch.zeros((2, ML - 1, R), dtype=torch.int32, device="cuda")
    x = torch.zeros((R, 512), dtype=torch.float32, device="cuda")
    N = 50

    def graph_us(fn):
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn(C.c_void_p(s.cuda_stream))
            s.synchronize()
            with torch.cuda.graph(g, stream=s):
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                for _ in range(N):
                    fn(st)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / 10 / N

    for pos in (8, 36, 70):
        for name, par in (("identity", np.tile(np.arange(K), B)),
                          ("shuffled", np.tile(np.array([1, 0, 0, 2]), B))):
            step = T(np.array([pos, 0, 0, 0], np.int32))
            parent = T(par.astype(np.int32))
            us = graph_us(lambda st: lib.qtx_beam_reorder(
                P(kc), P(vc), P(skc), P(svc), B, K, ML, NL, R * krow, R * vrow, R * ML, 1, P(step),
                P(parent), st))
            print(f"k_beam_reorder pos {pos:2d} {name:8s} {us:7.2f} us", flush=True)
    # the select advances its position: 50 launches walk positions 8 .. 57 (bounded writes)
    score = T(np.sort(-rng.uniform(0, 5, (B, K)).astype(np.float32), axis=1)[:, ::-1].reshape(-1))
    fin = torch.zeros((R,), dtype=torch.int32, device="cuda")
    ln = torch.zeros((R,), dtype=torch.int32, device="cuda")
    parent = torch.zeros((R,), dtype=torch.int32, device="cuda")
    step = T(np.array([8, 0, 0, 0], np.int32))
    logits[:, V - 1] = float("-inf")   # eos = V - 1 is never selected: every row stays live
    us = graph_us(lambda st: lib.qtx_beam_select(model.handle, P(logits), B, K, V - 1, V - 2, ML, P(step),
                                                P(score), P(fin), P(ln), P(parent), P(bp[0]),
                                                P(bp[1]), P(x), st))
    print(f"k_beam_select  B {B} beam {K} V {V}: {us:7.2f} us", flush=True)
    us = graph_us(lambda st: lib.qtx_debug_nop(st))
    print(f"empty kernel (dependent-launch floor): {us:7.2f} us", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["decode", "kernels"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-beam", action="store_true",
                    help="decode: the greedy lines only (this build against --lib, like for like)")
    a = ap.parse_args()
    decode(a) if a.what == "decode" else kernels(a)
