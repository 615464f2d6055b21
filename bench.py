"""bench.py — decoded tokens/s of int8 greedy decode on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline JSON line; with
--dump-outputs DIR it also writes what the last timed step computed (DIR/ids.npy, the
[batch, max_len] decoded ids in global sentence order, float32: ids < 2^24 are exact there);
the inputs are seeded, so two builds can be compared output for output.  --full adds
every side measurement and check listed below.

One "step" = one whole greedy decode of one batch of synthetic sentences: encoder, cross
K/V, max_len-1 = 71 KV-cached decoder steps, generator + argmax (the fixed loop of
reference/onnx_reference_inference.py:630, no EOS exit).  Workload at N=1 = BASELINE
config 2: batch 32 per GPU, source length <= 64 padded to 72.  For N > 1 one global batch
(batch x N sentences, or --global-batch, e.g. 2048 for BASELINE config 5) is partitioned
by source length over the ranks (one process per GPU, torchrun), each decoding its shard
with its own weight replica: no collective on the data path; RCCL carries
the barrier, the max-over-ranks of the elapsed time and, after the timed region (with
--full or --dump-outputs), the all-gather of the ids, which rank 0 checks against a
re-decoded sample (--full) or writes out (--dump-outputs).

With --full the printed JSON (rank 0) adds:
  ids_verified_vs_single_batch_sample, public_api_ms_per_decode, step, cfg4 / cfg5 / cfg1 lines
  (--no-cfg3 and --no-cpu-baseline leave legs of the --full run out)
  roofline     decode's dominant kernel, algorithmic bytes per launch / profiled avg duration
  roofline_encoder  the cfg3 encoder's FFN1 launch against the int8 MFMA peak (+ PMC traffic)
  cpu_baseline oracle/torch_port.py (the reference's fp32 fake-quant arithmetic in torch)
               on bounded samples on the host cores, rank 0 only
  cfg3_encoder encoder-only B=256 S=128 QuantLinear int8 ops/s vs the MFMA int8 peak
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))

PEAK_INT8_OPS = 256 * 4096 * 2 * 2.4e9     # dense int8 MFMA: 5.03e15 ops/s (MI355X_MICROARCH.md)
PEAK_HBM = 8.0e12                           # bytes/s (spec)
D, F = 512, 2048


def make_src(rng, B, S, max_src=64):
    """BOS + uniform tokens + EOS, lengths uniform in [8, max_src], padded with <blank>=2."""
    src = np.full((B, S), 2, np.int64)
    lens = rng.integers(8, max_src + 1, B)
    for b, n in enumerate(lens):
        src[b, 0] = 0
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        src[b, n - 1] = 1
    return src, lens


def encoder_gemm_ops(B, S, n_layers=6):
    M = B * S
    return n_layers * 2 * M * (3 * D * D + D * D + D * F + F * D)


def gemm_roofline_us(M):
    """Roofline bound of each QuantLinear launch of one encoder layer at M rows: max(MFMA
    time at the dense int8 peak, algorithmic HBM bytes at 8 TB/s).  Bytes: int8 A and W,
    fp32 row scales in/out, per-channel scale + bias, the int8 codes written; O and FFN2 also
    read the fp32 residual and write x (sublayer_connection.py:17) — the fp32 residual
    stream makes them HBM-bound whatever the GEMM does."""
    row = 4 * M                                   # one fp32 scale per row
    shapes = {  # name: (N, K, bytes besides A, W, sw/bias)
        "qkv_quant": (3 * D, D, 3 * (M * D + row)),
        "o_res_ln": (D, D, 2 * 4 * M * D + M * D + row + 8 * D),
        "ffn1_quant_onepass": (F, D, M * F + row),
        "ffn2_res_ln": (D, F, 2 * 4 * M * D + M * D + row + 8 * D)}
    out = {}
    for k, (N, K, extra) in shapes.items():
        by = M * K + row + N * K + 8 * N + extra
        out[k] = {"mfma_us": 2 * M * N * K / PEAK_INT8_OPS * 1e6, "hbm_us": by / PEAK_HBM * 1e6,
                  "alg_bytes": by}
        out[k]["bound_us"] = max(out[k]["mfma_us"], out[k]["hbm_us"])
        out[k]["bound"] = "mfma" if out[k]["mfma_us"] >= out[k]["hbm_us"] else "hbm"
    return out


# The decode step's dominant kernel class (most time per cfg2 step in the rocprofv3 kernel
# stats, profiles/r02q_bench_kernel_stats.md "by launch grid", B = 32 grids: 12 launches per
# step x 4.60 us = 55 us, ahead of cross-attention 31 and FFN2 33): the attention output
# projections O / Oc (attention.py:67 + sublayer_connection.py:17) — the fp32 context
# quantized per token in the prologue from its own row maximum (amode 3, round 5; the 8
# per-head partial maxima before), residual epilogue.
DOMINANT = "k_skinny<1, 4, 512, 8, 3, 2>"
DOMINANT_COPIES = 32   # rotating operand sets: 8 MB of weights, more than an XCD's 4 MB L2


def dominant_alg_bytes(B):
    """Algorithmic bytes of one O-projection decode launch: int8 W [512, 512] + fp32 context
    [B, 512] + per-channel scale and bias + fp32 residual in and out [B, 512]."""
    N, K = D, D
    return N * K + B * K * 4 + 2 * N * 4 + 2 * B * N * 4


def run_dominant(B, copies=DOMINANT_COPIES):
    """The decode step's dominant kernel at M = B rows, N = K = 512, as the step launches it
    (qtx_api.hip greedy_step_fused: amode A_F32R, EPI_RESIDUAL, out == res),
    over `copies` rotating operand sets so weights come from MALL as in the step, not from an
    L2-warm copy.  Returns (one(i): launch on operand set i % copies, on torch's current
    stream; keepalive)."""
    import ctypes as C

    import torch

    from qtx import _lib
    rng = np.random.default_rng(1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sets = []
    for _ in range(copies):
        ctx = rng.standard_normal((B, D)).astype(np.float32)
        sets.append((T(ctx), T(rng.integers(-127, 128, (D, D)).astype(np.int8)),
                     T(rng.standard_normal((B, D)).astype(np.float32))))
    sw = torch.full((D,), 0.01, device="cuda")
    bias = torch.zeros(D, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    S0 = C.c_void_p(0)
    L = _lib.lib(build=False)
    fn = L.qtx_skinny_linear

    def one(i):
        ctx, w, x = sets[i % copies]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = fn(3, S0, S0, P(ctx), D, S0, S0, S0, 0, P(w), P(sw), P(bias), B, D, D, 8, 2,
                P(x), P(x), S0, st)
        if rc:
            raise RuntimeError(f"qtx_skinny_linear: {L.qtx_last_error().decode()}")
    return one, (sets, sw, bias)


def nop():
    import ctypes as C

    import torch

    from qtx import _lib
    _lib.call("qtx_debug_nop", C.c_void_p(torch.cuda.current_stream().cuda_stream))


def graph_time(body, reps=5):
    """Microseconds of one replay of a hipGraph capturing body() (HIP events on the replay
    stream), the fastest of `reps` replays."""
    import torch
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        body()                                   # warm (and allocates nothing new)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            body()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            g.replay()
            e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1e3
        best = t if best is None else min(best, t)
    return best


def time_dominant(B, n=256):
    """(us per launch of the dominant kernel in a hipGraph chain of n launches, us per node
    of a chain of n empty kernels): HIP events on the replay stream."""
    one, keep = run_dominant(B)
    chain = graph_time(lambda: [one(i) for i in range(n)]) / n
    floor = graph_time(lambda: [nop() for _ in range(n)]) / n
    del keep
    return chain, floor


def step_alg_bytes(B, S, keys):
    """Algorithmic HBM bytes of one KV-cached decoder step (qtx_api.hip greedy_step_fused,
    50 kernels) with `keys` self-attention keys: every operand each kernel must read or
    write once — weights + scales/biases, K/V caches, fp32 activations between kernels,
    generator, logits, embedding row."""
    V = 4444
    lin = lambda N, K: N * K + 8 * N                      # int8 W + fp32 sw, bias
    x, x4 = B * D * 4, lambda n: B * n * 4                # fp32 [B, 512] / [B, n]
    per_layer = (lin(3 * D, D) + x + 8 * D + x4(3 * D)                      # LN + QKV
                 + x4(3 * D) + B * keys * (2 * D + 8) + B * (2 * D + 8) + x  # self-attn
                 + dominant_alg_bytes(B)                                   # O + residual
                 + lin(D, D) + x + 8 * D + x                              # LN + Qc
                 + x + B * S * (2 * D + 8) + B * S + x                    # cross-attn
                 + dominant_alg_bytes(B)                                   # Oc + residual
                 + lin(F, D) + x + 8 * D + x4(F)                          # LN + FFN1
                 + lin(D, F) + x4(F) + 2 * x)                             # FFN2 + residual
    tail = (V * D * 4 + V * 4 + x + 8 * D + x4(V)                          # final LN + generator
            + x4(V) + B * 8 + B * D * 4 + D * 4 + x)                      # argmax + embed
    return 6 * per_layer + tail


def pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC
    passes over it (tools/pmc_summary.py: 2 x FETCH_SIZE + WRITE_SIZE, the gfx950
    correction), or None when no profile names this kernel."""
    import glob
    for fn in sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_dominant.json")), reverse=True):
        with open(fn) as f:
            d = json.load(f)
        if d.get("kernel") == DOMINANT:
            return d.get("traffic_bytes_per_launch")
    return None


def profiler_dominant(B, alg):
    """A labelled side field, not the headline: the dominant kernel's average per-dispatch
    duration at the decode grid in the newest committed rocprofv3 kernel stats of this bench
    (tools/prof_summary.py "by launch grid" table) and the fraction it implies, with whether
    that profile was taken from the kernel sources this run is built from (its
    kernel_sources_sha16 line against tools/prof_summary.py's digest of csrc/ now), or None
    when no profile lists the kernel at that grid."""
    import glob
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from prof_summary import sources_sha16
    grid = f"{(D // 16) * 256}x{(B + 3) // 4}"          # 16 columns x 4 rows per workgroup
    for fn in sorted(glob.glob(os.path.join(REPO, "profiles", "*_bench_kernel_stats.md")), reverse=True):
        sha = None
        with open(fn) as f:
            for line in f:
                if line.startswith("kernel_sources_sha16:"):
                    sha = line.split(":", 1)[1].strip()
                cells = [c.strip() for c in line.split("|")]
                if len(cells) > 6 and DOMINANT in cells[1] and cells[2].startswith(grid + " "):
                    us = float(cells[5])
                    return {"source": os.path.relpath(fn, REPO), "avg_us": us,
                            "achieved": alg / (us * 1e-6) / 1e9, "frac": alg / (us * 1e-6) / PEAK_HBM,
                            "profiled_sources_sha16": sha,
                            "matches_current_sources": sha == sources_sha16() if sha else None,
                            "note": "rocprofv3 per-dispatch durations of the graph-replayed "
                                    "decode kernels; the profiler dispatches graph nodes one at "
                                    "a time, so they read longer than the live per-node time"}
    return None


# The encoder's north-star kernel (cfg3, BASELINE.json: >= 50 % of the int8-MFMA peak on the
# encoder QuantLinear GEMMs): the one-pass FFN1 (k_gemm_wsy, M = 32768, N = 2048, K = 512, the
# ReLU + per-token quantization epilogue), the launch furthest from its roofline.
ENC_DOMINANT = ("ffn1_quant_onepass", "k_gemm_wsy<0, 1>")


def pmc_encoder(kernel):
    """The newest committed rocprofv3 summary of the cfg3 encoder (tools/pmc_encoder.sh ->
    profiles/*_pmc_encoder.json) for one kernel: its profiled avg_us, corrected HBM bytes per
    dispatch (2 x FETCH_SIZE + WRITE_SIZE) and MfmaUtil, with the file it came from."""
    import glob
    for fn in sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_encoder.json")), reverse=True):
        with open(fn) as f:
            d = json.load(f)
        if kernel in d:
            k = d[kernel]
            return {"source": os.path.relpath(fn, REPO), "avg_us": k.get("avg_us"),
                    "hbm_bytes": k.get("hbm_read_bytes_corrected", 0) + k.get("hbm_write_bytes", 0),
                    "mfma_util_pct": k.get("MfmaUtil")}
    return None


def _quantized_rows(rng, M, K, relu=False):
    """int8 rows distributed as the encoder's activations: per-token absmax quantization
    (quant_linear.py:30-43) of Gaussian rows (LayerNorm outputs), or of ReLU'd Gaussian
    rows (the FFN hidden) — most codes small, the row maximum at 127."""
    g = rng.standard_normal((M, K), dtype=np.float32)
    if relu:
        g = np.maximum(g, 0.0)
    s = np.maximum(np.abs(g).max(1, keepdims=True), 1e-5) / 127.0
    return np.rint(g / s).astype(np.int8)


WS_RES_MAX_M = 8192       # qtx_api.hip ws_res_ok: O-projection weight-stationary below this M


def time_row_gemms(M=256 * 128, reps=10, ws=True, operands="encoder"):
    """The five QuantLinear launches of one cfg3 encoder layer through qtx_linear_rows on
    synthetic int8 operands (QKV + per-token quant, O + residual + LN + quant, FFN1 row-max
    pass, FFN1 ReLU + quant pass, FFN2 + residual + LN + quant): (us per launch, ops).
    ws: the Q/K/V and FFN1 launches on the weight-stationary kernel (kp = 2), as the encoder
    runs them at this M (csrc/qtx_api.hip rowgemm); O and FFN2 on the KP row GEMM.
    operands: "encoder" = activations per-token quantized from Gaussian (ReLU'd for FFN2)
    rows and weights uniform over [-127, 127] (what per-channel quantization of the
    Xavier-uniform synthetic weights gives) — the encoder's own operand statistics;
    "uniform" = every operand uniform over [-127, 127], the MFMA power worst case (the
    matrix-core clock drops with operand toggling)."""
    import ctypes as C

    import torch

    from qtx import _lib
    L = _lib.lib(build=False)
    rng = np.random.default_rng(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if operands == "uniform":
        a512 = T(rng.integers(-127, 128, (M, D)).astype(np.int8))
        a2048 = T(rng.integers(-127, 128, (M, F)).astype(np.int8))
    else:
        a512 = T(_quantized_rows(rng, M, D))
        a2048 = T(_quantized_rows(rng, M, F, relu=True))
    sa = torch.full((M,), 0.01, device="cuda")
    W = {nk: T(rng.integers(-127, 128, nk).astype(np.int8)) for nk in [(3 * D, D), (D, D), (F, D), (D, F)]}
    sw = torch.full((F,), 0.01, device="cuda")
    bias = torch.zeros(F, device="cuda")
    out8 = torch.empty((M * F,), dtype=torch.int8, device="cuda")
    os_ = torch.empty((4 * M,), device="cuda")
    x = torch.randn((M, D), device="cuda")
    lna, lnb = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    pm = torch.full((4, M), 3.0, device="cuda")
    gx = torch.empty((32 * M + 2048) // 4, device="cuda")
    # the encoder runs the KP instances (csrc/qtx_api.hip encoder_run: kp = 1): weights
    # packed by qtx_pack_w_kp, A in the KP layout (random bytes: any layout of them is)
    kps = {}
    for (N, K), w in list(W.items()):
        wk = torch.empty_like(w)
        # Q/K/V and FFN1 weight-stationary (qtx_api.hip rowgemm); O too below the M bound of
        # qtx_api.hip ws_res_ok (the same environment override, the same default)
        o_ws = 2048 <= M < int(os.environ.get("QTX_WS_RES_MAX_M", str(WS_RES_MAX_M)))
        kps[(N, K)] = 2 if (ws and K == D and (N != D or o_ws)) else 1
        if kps[(N, K)] == 2 and N in (3 * D, F) and os.environ.get("QTX_WS32", "0") != "0":
            kps[(N, K)] = 4                  # W in the WS32 layout (diagnostic library, QTX_WS32)
        _lib.call({1: "qtx_pack_w_kp", 2: "qtx_pack_w_ws", 4: "qtx_debug_pack_w_ws32"}[kps[(N, K)]],
                  C.c_void_p(w.data_ptr()), N, K, C.c_void_p(wk.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        W[(N, K)] = wk
    cases = [("qkv_quant", 3 * D, D, a512, dict(epi=0, out8=out8, ldo8=D, o8_ts=M * D, os=os_, os_ts=M)),
             ("o_res_ln", D, D, a512, dict(epi=1, res=x, xout=x, ln_a=lna, ln_b=lnb, lnq=out8, lns=os_)),
             # FFN1 in one pass (kp = 3: the slices' row maxima exchanged in-launch; pmax_out
             # is the exchange scratch), as the encoder runs it
             ("ffn1_quant_onepass", F, D, a512, dict(epi=3, kp=5 if kps[(F, D)] == 4 else 3, pmax_out=gx,
                                                     out8=out8, ldo8=F, os=os_)),
             ("ffn2_res_ln", D, F, a2048, dict(epi=1, res=x, xout=x, ln_a=lna, ln_b=lnb, lnq=out8, lns=os_))]
    if os.environ.get("QTX_BENCH_FFN1_2PASS", "0") == "1":
        # FFN1 as two weight-stationary passes (row maxima, then ReLU + quant from them)
        cases[2:3] = [("ffn1_rowmax", F, D, a512, dict(epi=2, pmax_out=pm)),
                      ("ffn1_quant", F, D, a512, dict(epi=3, pmax_in=pm, pmax_n=4, out8=out8, ldo8=F, os=os_))]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for name, N, K, a, kw in cases:
        args = _lib.RowGemm()
        for k, v in {**dict(A=a, sa=sa, W=W[(N, K)], sw=sw, bias=bias, M=M, N=N, K=K, kp=kps[(N, K)]), **kw}.items():
            setattr(args, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
        for _ in range(3):
            _lib.call("qtx_linear_rows", C.byref(args), st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            L.qtx_linear_rows(C.byref(args), st)
        e1.record()
        torch.cuda.synchronize()
        res[name] = (e0.elapsed_time(e1) / reps * 1e3, 2 * M * N * K)
    return res


def time_encoder_cfg3(model=None, B=256, S=128, n=5):
    """Seconds per encoder-only forward at B x S (BASELINE cfg3), HIP events."""
    import torch
    if model is None:
        from qtx.model import QtxModel
        from qtx.weights import synthetic_state_dict
        model = QtxModel(synthetic_state_dict(20241223))
    xs = torch.randn((B, S, D), device="cuda")
    mk = torch.ones((B, S), dtype=torch.uint8, device="cuda")
    for _ in range(2):
        model.encode(xs, mk)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        model.encode(xs, mk)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / n


def time_decode(model, B, S, L, steps=3, seed=1000):
    """ms per greedy decode (encoder + L-1 steps) of B synthetic sentences."""
    import torch
    src, _ = make_src(np.random.default_rng(seed), B, S)
    srcd = torch.from_numpy(src).cuda()
    maskd = (srcd != 2).to(torch.uint8)
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")
    for _ in range(2):
        model.greedy(srcd, maskd, max_len=L, start=0, out=ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.greedy(srcd, maskd, max_len=L, start=0, out=ids)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def workload_name(args, G, world):
    """The BASELINE.json config a run measures (cfg2: 32 sentences per GPU; cfg4: the same
    with int4 weights; cfg5: 2048 sentences over the ranks)."""
    if args.weight_bits == 4:
        return "cfg4" if G == 32 * world else "int4 custom"
    if G == 2048:
        return "cfg5"
    return "cfg2" if G == 32 * world else "custom"


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


ALL_CPUS_STEPS, ALL_CPUS_TIMEOUT_S = 8, 40


def all_cpus_leg(B, S, seed):
    """BASELINE.md §3's plan, torch.set_num_threads(os.cpu_count()): the cfg2 batch decoded
    (ALL_CPUS_STEPS steps, a bounded sample) on every CPU the host reports, in a child
    process with a time limit — on the GPU box os.cpu_count() is the whole shared host while
    the job's CPU share is OMP_NUM_THREADS = 16, and that many threads on the share can stall
    (round 6: the in-process leg ran past the box's 180 s silence limit).
    Returns (threads, decoded tokens/s or None, note)."""
    import subprocess
    allc = os.cpu_count() or 1
    code = ("import os,sys,time,numpy as np,torch;sys.path[:0]=[%r,%r];"
            "torch.set_num_threads(%d);from bench import make_src;"
            "from oracle.torch_port import TorchPortModel;"
            "from qtx.weights import synthetic_state_dict;"
            "tp=TorchPortModel(synthetic_state_dict(20241223));"
            "src,_=make_src(np.random.default_rng(%d),%d,%d);"
            "m=torch.from_numpy((src!=2)[:,None,:]);s=torch.from_numpy(src);"
            "tp.greedy_decode(s[:2],m[:2],4);t0=time.perf_counter();"
            "tp.greedy_decode(s,m,%d);print((time.perf_counter()-t0))"
            % (REPO, os.path.join(REPO, "onnx-transformer_amd"), allc, seed, B, S, ALL_CPUS_STEPS + 1))
    env = dict(os.environ, OMP_NUM_THREADS=str(allc))
    note = (f"cfg2 batch ({B} sentences), {ALL_CPUS_STEPS} greedy steps, torch.set_num_threads"
            f"(os.cpu_count() = {allc}) in a child process (BASELINE.md §3's plan); the value "
            f"above runs on the per-GPU CPU share (OMP_NUM_THREADS)")
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                           env=env, timeout=ALL_CPUS_TIMEOUT_S)
        if r.returncode == 0:
            return allc, B * ALL_CPUS_STEPS / float(r.stdout.strip().splitlines()[-1]), note
        return allc, None, note + f"; failed: {r.stderr.strip()[-200:]}"
    except subprocess.TimeoutExpired:
        return allc, None, note + f"; did not finish in {ALL_CPUS_TIMEOUT_S} s: that many " \
                                  "threads on this job's CPU quota (cgroup cpu.max 16 CPUs on the GPU box) " \
                                  "stall; profiles/r06_all_cpus_probe.log: 16 threads 801 tok/s, 64 threads " \
                                  "246 tok/s (4-step samples), 256 threads no 2-sentence warm-up in 95 s"


def cpu_baseline(sd, B=32, S=72, max_len=72, seed=7):
    """The reference's CPU arithmetic (fp32 fake-quant W8A8, oracle/torch_port.py: torch on
    the host cores, KV-cached) on bounded samples, rank 0 only: cfg2 (B=32 decode, the
    headline unit), cfg1 (B=1 decode) and cfg3 (encoder B=256 S=128, int8-op rate)."""
    import torch

    from oracle.torch_port import TorchPortModel
    threads = torch.get_num_threads()
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = None
    tp = TorchPortModel(sd)
    src, _ = make_src(np.random.default_rng(seed), B, S)
    mask = torch.from_numpy((src != 2)[:, None, :])
    srct = torch.from_numpy(src)
    tp.greedy_decode(srct[:2], mask[:2], 4)                     # warm the thread pool
    t0 = time.perf_counter()
    tp.greedy_decode(srct, mask, max_len)
    t2 = time.perf_counter() - t0
    t0 = time.perf_counter()
    tp.greedy_decode(srct[:1], mask[:1], max_len)
    t1 = time.perf_counter() - t0
    xe = torch.randn((256, 128, D))
    me = torch.ones((256, 1, 128), dtype=torch.bool)
    t0 = time.perf_counter()
    tp.encode(xe, me)
    t3 = time.perf_counter() - t0
    allc, allc_rate, allc_note = all_cpus_leg(B, S, seed)
    return {"value": B * (max_len - 1) / t2, "unit": "decoded tokens/s", "cores": int(threads),
            "kind": "port",
            "sample": f"oracle/torch_port.py (the reference's fp32 fake-quant arithmetic in "
                      f"torch, KV-cached) on {threads} threads of '{cpu_model()}' (torch's "
                      f"thread count = OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')}, this "
                      f"host's CPU share per GPU; os.cpu_count()={os.cpu_count()} is the whole "
                      f"host, {affinity} CPUs in this process's affinity mask): cfg2 greedy "
                      f"decode B={B}, S={S}, {max_len - 1} steps in {t2:.1f}s",
            "all_cpus": {"threads": int(allc), "value": allc_rate, "note": allc_note},
            "cfg1_b1_decode_tokens_per_s": (max_len - 1) / t1,
            "cfg3_encoder_s": t3,
            "cfg3_encoder_int8_ops_per_s": encoder_gemm_ops(256, 128) / t3}


def main():
    t_start = time.perf_counter()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="sentences per GPU (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="total sentences over all ranks (cfg5: 2048); default batch x world")
    ap.add_argument("--src-len", type=int, default=72)
    ap.add_argument("--max-len", type=int, default=72)
    ap.add_argument("--weight-bits", type=int, default=8)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's decoded ids to DIR/ids.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the side measurements and checks (roofline, step, public API, "
                         "cfg1/3/4/5, CPU baseline, id verification)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-cfg3", action="store_true", help="with --full: skip the cfg3/4/5/1 lines")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # RCCL ("nccl") in production: one rank per GPU.  QTX_BENCH_BACKEND=gloo rehearses the
    # multi-rank flow (sharding, timing reduction, id gather, verification) with several
    # ranks sharing the GPUs there are, e.g. two ranks on a one-GPU box.
    backend = os.environ.get("QTX_BENCH_BACKEND", "nccl")
    dev_index = local if backend == "nccl" else local % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    coll_dev = "cuda" if backend == "nccl" else "cpu"
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    from qtx import _build
    if rank == 0:
        _build.build()
    if world > 1:
        dist.barrier()
    from qtx.decode import gather_ids, greedy_decode, length_sorted_shards
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict

    sd = synthetic_state_dict(20241223)
    model = QtxModel(sd, ModelConfig(weight_bits=args.weight_bits))
    S, L = args.src_len, args.max_len
    # one global batch (same seed on every rank), partitioned by source length:
    # each rank decodes its shard; no collective on the data path
    G = args.global_batch or args.batch * world
    gsrc, glens = make_src(np.random.default_rng(20241223), G, S)
    idx = length_sorted_shards(glens, world)[rank]
    B = len(idx)
    srcd = torch.from_numpy(gsrc[idx]).cuda()
    maskd = (srcd != 2).to(torch.uint8)
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")

    def step():
        model.greedy(srcd, maskd, max_len=L, start=0, out=ids)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    tokens = G * (L - 1) * args.steps
    value = tokens / dt

    # after the timed region (--full or --dump-outputs): gather every rank's ids into global
    # order; --dump-outputs writes them, and with --full rank 0 re-decodes a sample of
    # sentences from every shard in one batch of its own (per-token quantization: a
    # sentence's tokens do not depend on its batch)
    want_ids = args.full or args.dump_outputs is not None
    allids = gather_ids(dist, ids.to(coll_dev), idx, G, world) if world > 1 and want_ids else None
    verified = None
    if rank == 0 and want_ids:
        if allids is None:
            allids = np.full((G, L), -1, np.int64)
            allids[idx] = ids.cpu().numpy()
    if rank == 0 and args.dump_outputs is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        rows = allids
        if rows.size * 4 > 64 << 20:            # a fixed, seeded sample of the sentences
            keep = np.random.default_rng(0).choice(G, (64 << 20) // (4 * L), replace=False)
            rows = rows[np.sort(keep)]
        np.save(os.path.join(args.dump_outputs, "ids.npy"), rows.astype(np.float32))
    if rank == 0 and args.full:
        shards = length_sorted_shards(glens, world)
        pick = np.unique(np.concatenate([sh[[0, len(sh) // 2, -1]] for sh in shards if len(sh)]))
        ref = greedy_decode(model, gsrc[pick], (gsrc[pick] != 2)[:, None, :], L, 0)
        verified = bool((allids >= 0).all() and np.array_equal(ref, allids[pick]))

    def progress(msg):      # stderr, so a long run is visibly alive (stdout: the JSON line only)
        print(f"bench: {msg} ({time.perf_counter() - t_start:.0f} s since start)", file=sys.stderr, flush=True)

    # the headline: all a plain run prints
    head = {"metric": "decoded tokens/sec IWSLT14 de-en int8 greedy "
                      f"(batch {G} over {world} GPU, {L - 1} steps)",
            "value": value, "unit": "tokens/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak" if not args.global_batch else "strong",
            "vs_baseline": None,
            "dtype": "int8" if args.weight_bits == 8 else "int4w-int8a",
            "data": "synthetic (seeded src ids, random-init weights of the reference architecture)",
            "config": {"workload": f"{workload_name(args, G, world)}: greedy decode, src<=64 "
                                   f"padded to {S}, max_len={L}, {G} sentences length-sorted "
                                   f"over {world} rank(s)",
                       "global_batch": G, "per_gpu_batch": B, "seq_len": S,
                       "parallelism": f"sentence-shard x{world}"}}
    if rank == 0 and not args.full:
        print(json.dumps(head))
    if rank == 0 and args.full:
        progress(f"timed region done: {value:.0f} tokens/s")
        Bd = min(B, 32)
        chain_us, nop_us = time_dominant(Bd)
        # per-launch time = one node of a dependent hipGraph chain, as the decode step runs
        # it (its launch boundary included: conservative).  rocprofv3's per-dispatch
        # durations of graph-replayed nodes are inflated by the profiler (an empty kernel
        # reads 4.6 us there, 1.6 us per node live: profiles/r03b_dominant_timing.md)
        alg = dominant_alg_bytes(Bd)
        # achieved / frac from THIS run's measurement: the live chain, us per
        # node with its launch boundary included (conservative); the committed rocprofv3
        # per-dispatch view is a labelled side field ("profiler"), flagged when it was taken
        # from other kernel sources than the ones this run is built from
        prof = profiler_dominant(Bd, alg)
        kt = chain_us * 1e-6
        roof = {"kernel": f"{DOMINANT}: decode O / Oc projection (M={Bd}, N={D}, K={D}, int8, "
                          "fp32 context quantized per token in the prologue, residual epilogue)",
                "bound": "hbm", "achieved": alg / kt / 1e9, "peak": PEAK_HBM / 1e9,
                "unit": "GB/s", "frac": alg / kt / PEAK_HBM, "traffic": pmc_traffic(),
                "avg_us": chain_us, "alg_bytes_per_launch": alg,
                "empty_node_us": nop_us, "marginal_us": chain_us - nop_us,
                "method": f"live, this run: hipGraph chain of 256 dependent launches over "
                          f"{DOMINANT_COPIES} rotating operand sets at the decode grid, HIP "
                          "events on the replay stream: us per node (launch boundary "
                          "included); empty_node_us = the same chain of empty kernels",
                "profiler": prof}
        # the whole decode step: (decode of max_len - 1 steps) - (decode of 1 step), per step
        t_full = time_decode(model, Bd, S, L)
        t_one = time_decode(model, Bd, S, 2)
        step_us = (t_full - t_one) / (L - 2) * 1e6
        sb = np.mean([step_alg_bytes(Bd, S, k) for k in range(2, L)])
        step = {"B": Bd, "us": step_us, "alg_bytes": float(sb), "achieved": sb / step_us / 1e3,
                "unit": "GB/s", "frac": sb / (step_us * 1e-6) / PEAK_HBM, "kernels": 50,
                "empty_node_us": nop_us, "chain_floor_us": 50 * nop_us,
                "note": "us = (decode of 71 steps - decode of 1 step) / 70; alg_bytes averaged "
                        "over the 70 steps' self-attention key counts"}
        # the public API path (numpy in, numpy out, fresh buffers each call)
        pub = []
        for _ in range(3):
            t0 = time.perf_counter()
            greedy_decode(model, gsrc[idx], (gsrc[idx] != 2)[:, None, :], L, 0)
            pub.append(time.perf_counter() - t0)
        out = {**head,
               "ids_verified_vs_single_batch_sample": verified,
               "public_api_ms_per_decode": min(pub) * 1e3,
               "roofline": roof, "step": step}
        if not args.no_cfg3:
            progress("roofline / step / public API done; cfg3 encoder next")
            Bc, Sc = 256, 128
            te = time_encoder_cfg3(model, Bc, Sc)
            ops = encoder_gemm_ops(Bc, Sc)
            g = time_row_gemms(Bc * Sc)
            gemm_us = sum(t for t, _ in g.values())
            gemm_ops = sum(o for _, (_, o) in g.items())
            out["cfg3_encoder"] = {
                "B": Bc, "S": Sc, "ms": te * 1e3, "quantlinear_int8_ops": ops,
                "whole_encoder_ops_per_s": ops / te,
                "frac_of_int8_peak_whole_encoder": ops / te / PEAK_INT8_OPS,
                # the layer's QuantLinear launches alone, as the encoder runs them (WS / KP
                # instances, FFN1 in one pass), on operands with the encoder's statistics
                # (per-token quantized activations; uniform random bytes measured the same
                # within 2 %, profiles/r02j_pmc_encoder.json's note)
                "gemm_us_per_layer": {k: round(t, 1) for k, (t, _) in g.items()},
                "frac_of_int8_peak_quantlinear_gemms": gemm_ops / (gemm_us * 1e-6) / PEAK_INT8_OPS}
            # each launch against its own roofline (max of MFMA and HBM time): O and FFN2
            # carry the fp32 residual stream, so the int8 peak fraction the layer can reach
            # at all is sum(ops) / sum(bounds) / peak (0.57 at 8 TB/s)
            rf = gemm_roofline_us(Bc * Sc)
            bound_us = sum(r["bound_us"] for r in rf.values())
            out["cfg3_encoder"]["roofline_us_per_layer"] = {
                k: {"bound": r["bound"], "bound_us": round(r["bound_us"], 1),
                    "frac": round(r["bound_us"] / g[k][0], 3)} for k, r in rf.items()}
            out["cfg3_encoder"]["frac_of_roofline_quantlinear_gemms"] = bound_us / gemm_us
            out["cfg3_encoder"]["int8_peak_frac_attainable"] = gemm_ops / (bound_us * 1e-6) / PEAK_INT8_OPS
            # the encoder's north-star kernel against the int8 MFMA peak: live launch time
            # (HIP events, this run) and the committed profiler view with its PMC HBM traffic
            name, kname = ENC_DOMINANT
            us, ops1 = g.get(name, (float("nan"), 0))
            pe = pmc_encoder(kname)
            ab = rf[name]["alg_bytes"]
            out["roofline_encoder"] = {
                "kernel": f"{kname}: cfg3 FFN1 one pass (M={Bc * Sc}, N={F}, K={D}, int8, ReLU + "
                          "per-token quantization over all 2048 columns in the epilogue)",
                "bound": rf[name]["bound"], "achieved": ops1 / (us * 1e-6) / 1e12,
                "peak": PEAK_INT8_OPS / 1e12, "unit": "TOP/s (int8)",
                "frac": ops1 / (us * 1e-6) / PEAK_INT8_OPS, "avg_us": us,
                "alg_bytes_per_launch": ab,
                "traffic": pe["hbm_bytes"] if pe else None,
                "traffic_over_alg": (pe["hbm_bytes"] / ab) if pe else None,
                "profiler": ({"source": pe["source"], "avg_us": pe["avg_us"],
                              "frac": ops1 / (pe["avg_us"] * 1e-6) / PEAK_INT8_OPS,
                              "mfma_util_pct": pe["mfma_util_pct"]} if pe else None),
                "method": "the launch alone at cfg3's M as the encoder runs it (10 launches, HIP "
                          "events); profiler = the newest profiles/*_pmc_encoder.json"}
            # BASELINE configs 4 and 5 (secondary lines): int4 weights at B=32, and the
            # per-GPU shard of the 8-GPU config (B=2048 / 8 = 256 sentences)
            m4 = QtxModel(sd, ModelConfig(weight_bits=4))
            t4 = time_decode(m4, 32, S, L)
            out["cfg4_int4_decode"] = {"B": 32, "ms": t4 * 1e3, "tokens_per_s": 32 * (L - 1) / t4}
            del m4
            t5 = time_decode(model, 256, S, L)
            out["cfg5_per_gpu_decode"] = {"B": 256, "ms": t5 * 1e3, "tokens_per_s": 256 * (L - 1) / t5}
            # cfg1's shape (one sentence, the reference's own CPU-runnable case) on the GPU:
            # the latency of one greedy decode, beside cpu_baseline's cfg1 leg
            t1 = time_decode(model, 1, S, L)
            out["cfg1_b1_decode"] = {"B": 1, "ms": t1 * 1e3, "tokens_per_s": (L - 1) / t1}
        if not args.no_cpu_baseline and world == 1:
            progress("GPU lines done; CPU baseline next")
            out["cpu_baseline"] = cpu_baseline(sd)
            progress("CPU baseline done")
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
