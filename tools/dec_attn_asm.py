"""Where k_dec_attn's score phase sits in the code object, as a markdown table, for two device
assemblies of csrc/qtx_decode.hip (tools/kernarg_table.py --emit writes one with the
product's flags):

    python tools/dec_attn_asm.py parent.s new.s

Columns per assembly, instruction indices counted from the kernel's real entry as in
tools/kernarg_table.py: `last ld` = the last global load; `score` = the first instruction of
the dot products (the first v_mfma_i32, or the first v_dot4 where the kernel has no MFMA);
`lds` / `bar` = LDS instructions and s_barriers ahead of the first qexp (its log2(e)
constant 0x3fb8aa3b); `len` = instructions ahead of the first qexp; `vgpr` / `scr` = the
kernel descriptor's VGPR count and private segment size.
"""
import re
import sys

from kernarg_table import demangle

KERNELS = ["k_dec_attn<true, 1>", "k_dec_attn<true, 3>", "k_dec_attn<true, 5>", "k_dec_attn<false, 5>"]


def parse(path):
    """{mangled name: (last load, first score op, lds, barriers, length, vgprs, scratch)}"""
    body, meta, cur = {}, {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                cur = m.group(1)
                meta[cur] = {}
                continue
            m = re.match(r"\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|user_sgpr_kernarg_preload_length) (\d+)", line)
            if m and cur in meta:
                meta[cur][m.group(1)] = int(m.group(2))
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
    for k, md in meta.items():
        ins = body.get(k, [])
        if md.get("user_sgpr_kernarg_preload_length") and ".p2align\t8" in ins:
            ins = ins[ins.index(".p2align\t8") + 1:]
        ins = [i for i in ins if not i.startswith(".")]
        qexp = next((i for i, s in enumerate(ins) if "0x3fb8aa3b" in s), None)
        if qexp is None:
            continue
        head = ins[:qexp]
        loads = [i for i, s in enumerate(head) if s.startswith("global_load")]
        score = next((i for i, s in enumerate(head) if s.startswith("v_mfma_i32")), None)
        if score is None:
            score = next((i for i, s in enumerate(head) if s.startswith("v_dot4")), -1)
        out[k] = (loads[-1] if loads else -1, score, sum(s.startswith("ds_") for s in head),
                  sum(s.startswith("s_barrier") for s in head), qexp,
                  md.get("next_free_vgpr", -1), md.get("private_segment_fixed_size", -1))
    return out


def main():
    tabs = [parse(p) for p in sys.argv[1:3]]
    names = demangle(sorted(set(tabs[0]) | set(tabs[1])))
    cols = "last ld | score | lds | bar | len | vgpr | scr"
    print(f"| kernel | parent: {cols} | new: {cols} |")
    print("|---|" + "---:|" * 14)
    for pat in KERNELS:
        cells = []
        for tab in tabs:
            hit = [v for k, v in tab.items() if pat in names[k]]
            assert len(hit) == 1, (pat, len(hit))
            cells += [str(x) for x in hit[0]]
        print(f"| `{pat}` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
