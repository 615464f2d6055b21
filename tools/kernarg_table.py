"""Kernel-argument preload evidence from the code object, as a markdown table: per decode-step
kernel instantiation the preload length and where its first load phase sits, for two device
assemblies of csrc/qtx_decode.hip (e.g. the parent commit's and this tree's).

    python tools/kernarg_table.py --emit new.s          # this tree, the product's flags
    python tools/kernarg_table.py parent.s new.s > profiles/r07_kernarg_preload.md

Columns per assembly: `pre` = .amdhsa_user_sgpr_kernarg_preload_length (dwords); `first` /
`last` = instruction index, counted from the kernel's real entry (past the 256-byte block that
loads the arguments for firmware without preload), of the first global load and of the last
global load of the first load phase (the loads ahead of the first s_barrier); `wait` = whether
an s_waitcnt on lgkmcnt stands ahead of the first global load, and in brackets how many stand
ahead of the last one.
"""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the step's launches (qtx_api.hip greedy_step_fused, qtx_decode.hip skinny_mode) with 8-bit
# weights; NIT of k_dec_attn = ceil(rows staged / 16): 72 positions -> 1 .. 5
STEP_KERNELS = [
    ("32", "LN+QKV", "k_skinny_wide<4, 8, 1, 0>"),
    ("32", "O / Oc + res", "k_skinny<1, 4, 512, 8, 3, 2>"),
    ("32", "LN+Qc", "k_skinny<1, 4, 512, 8, 1, 0>"),
    ("32", "LN+FFN1+relu", "k_skinny_wide<4, 8, 1, 1>"),
    ("32", "FFN2 + res", "k_skinny8_ffn2<true>"),
    ("256", "LN+QKV, LN+Qc", "k_skinny_wide<8, 8, 1, 0>"),
    ("256", "O / Oc + res", "k_skinny_wide<8, 8, 3, 2>"),
    ("256", "LN+FFN1+relu", "k_skinny_wide<8, 8, 1, 1>"),
    ("256", "h quantizer", "k_quant_h2048("),
    ("256", "FFN2 + res", "k_skinny<1, 16, 2048, 8, 0, 2>"),
    ("both", "self-attention", "k_dec_attn<true, 1>"),
    ("both", "self-attention", "k_dec_attn<true, 3>"),
    ("both", "self-attention", "k_dec_attn<true, 5>"),
    ("both", "cross-attention", "k_dec_attn<false, 5>"),
    ("both", "generator", "k_generator_mfma("),
    ("both", "argmax + embedding", "k_argmax_embed("),
]


def emit(out):
    sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))
    from qtx import _build
    src = os.path.join(_build.CSRC, "qtx_decode.hip")
    subprocess.run([_build.hipcc(), *_build.compile_flags(src), "-S", "--cuda-device-only",
                    "-o", out, src], check=True)


def demangle(names):
    sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))
    from qtx import _build
    filt = os.path.join(os.path.dirname(os.path.realpath(_build.hipcc())), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def parse(path):
    """{mangled name: (preload length, first, last, waits before first, waits before last)}"""
    pre, body, cur = {}, {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                cur = m.group(1)
                pre.setdefault(cur, 0)
                continue
            m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
            if m and cur:
                pre[cur] = int(m.group(1))
                continue
            m = re.match(r"(_Z\w+):", line)
            if m:
                cur = m.group(1)
                body[cur] = []
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
            elif cur in body and (re.match(r"\t[a-z]", line) or ".p2align\t8" in line):
                body[cur].append(line.strip())
    out = {}
    for k, n in pre.items():
        ins = body.get(k, [])
        if n and ".p2align\t8" in ins:
            ins = ins[ins.index(".p2align\t8") + 1:]
        ins = [i for i in ins if not i.startswith(".")]
        end = next((i for i, s in enumerate(ins) if s.startswith("s_barrier")), len(ins))
        loads = [i for i, s in enumerate(ins[:end]) if s.startswith("global_load")]
        if not loads:
            continue
        waits = [i for i, s in enumerate(ins[:end]) if s.startswith("s_waitcnt") and "lgkmcnt" in s]
        out[k] = (n, loads[0], loads[-1], sum(w < loads[0] for w in waits), sum(w < loads[-1] for w in waits))
    return out


def main():
    if sys.argv[1] == "--emit":
        return emit(sys.argv[2])
    tabs = [parse(p) for p in sys.argv[1:3]]
    names = demangle(sorted(set(tabs[0]) | set(tabs[1])))

    def find(tab, pat):
        hit = [v for k, v in tab.items() if pat in names[k]]
        assert len(hit) == 1, (pat, len(hit))
        return hit[0]
    print("| B | launch | kernel | parent: pre | first | last | wait | new: pre | first | last | wait |")
    print("|---|---|---|---:|---:|---:|---|---:|---:|---:|---|")
    for b, what, pat in STEP_KERNELS:
        cells = []
        for tab in tabs:
            n, first, last, w0, w1 = find(tab, pat)
            cells += [str(n), str(first), str(last), f"{'yes' if w0 else 'no'} ({w1})"]
        print(f"| {b} | {what} | `{pat.rstrip('(')}` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
