"""Instruction counts on the critical paths of the decode step's kernels, as markdown, for two
device assemblies of csrc/qtx_decode.hip (tools/kernarg_table.py --emit writes one with the
product's flags):

    python tools/step_asm.py parent.s new.s

Skinny GEMMs: `quant` = instructions from the first wait on a row's loads (the first
s_waitcnt vmcnt) to the first ds_write of the codes, `valu` / `salu` / `br` = the vector,
scalar and branch instructions among them; `bar` = s_barrier in the kernel.  Attention:
`head` / `br` = instructions and s_cbranch ahead of the first MFMA (cold blocks laid out
behind the kernel's end are not ahead of it), `lds` = LDS instructions in the kernel.  All:
`scr` = private segment size, `pre` = kernel-argument preload length."""
import re
import sys

from dec_attn_asm import demangle

SKINNY = ["k_skinny<1, 4, 512, 8, 3, 2>", "k_skinny<1, 4, 512, 8, 1, 0>", "k_skinny_wide<4, 8, 1, 0>",
          "k_skinny_wide<4, 8, 1, 1>", "k_skinny8_ffn2<true>"]
ATTN = ["k_dec_attn<true, 1>", "k_dec_attn<true, 3>", "k_dec_attn<true, 5>", "k_dec_attn<false, 5>"]


def parse(path):
    """{mangled name: (instructions, scratch, preload length)}"""
    body, meta, cur = {}, {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                cur = m.group(1)
                meta[cur] = {}
                continue
            m = re.match(r"\s*\.amdhsa_(private_segment_fixed_size|user_sgpr_kernarg_preload_length) (\d+)", line)
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
                body[cur].append(line.split(";")[0].strip())
    out = {}
    for k, md in meta.items():
        ins, pre = body.get(k, []), md.get("user_sgpr_kernarg_preload_length", 0)
        if pre and ".p2align\t8" in ins:          # counted from the kernel's real entry
            ins = ins[ins.index(".p2align\t8") + 1:]
        out[k] = ([i for i in ins if not i.startswith(".")], md.get("private_segment_fixed_size", -1), pre)
    return out


def one(tab, names, pat):
    hit = [v for k, v in tab.items() if names[k].startswith(pat + "(")]
    assert len(hit) == 1, (pat, len(hit))
    return hit[0]


def skinny_row(ins, scr, pre):
    w = next(i for i, s in enumerate(ins) if s.startswith("s_waitcnt vmcnt"))
    # (the codes are packed by v_perm_b32: a ds_write ahead of the first one is not theirs)
    p = next(i for i, s in enumerate(ins) if s.startswith("v_perm_b32"))
    d = next(i for i, s in enumerate(ins) if i > p and s.startswith("ds_write"))
    seg = ins[w:d]
    return [d - w, sum(s.startswith("v_") for s in seg),
            sum(s.startswith("s_") and not s.startswith(("s_waitcnt", "s_nop", "s_cbranch")) for s in seg),
            sum(s.startswith("s_cbranch") for s in seg), sum(s.startswith("s_barrier") for s in ins), scr, pre]


def attn_row(ins, scr, pre):
    end = next(i for i, s in enumerate(ins) if s.startswith("s_endpgm"))
    m = next(i for i, s in enumerate(ins) if s.startswith("v_mfma"))
    return [m, sum(s.startswith("s_cbranch") for s in ins[:m]), sum(s.startswith("ds_") for s in ins),
            len(ins), len(ins) - end - 1, scr, pre]


def table(tabs, names, pats, fn, cols):
    print(f"| kernel | parent: {cols} | new: {cols} |")
    print("|---|" + "---:|" * (2 * len(cols.split("|"))))
    for pat in pats:
        cells = []
        for tab, nm in zip(tabs, names):
            cells += [str(x) for x in fn(*one(tab, nm, pat))]
        print(f"| `{pat}` | " + " | ".join(cells) + " |")
    print()


def main():
    tabs = [parse(p) for p in sys.argv[1:3]]
    names = [{k: re.sub(r"^void qtx::|^qtx::", "", v) for k, v in demangle(sorted(t)).items()} for t in tabs]
    table(tabs, names, SKINNY, skinny_row, "quant | valu | salu | br | bar | scr | pre")
    table(tabs, names, ATTN, attn_row, "head | br | lds | all | cold | scr | pre")
    worst = max(v[1] for t in tabs for v in t.values())
    print(f"largest private segment of any kernel in either file: {worst} bytes")


if __name__ == "__main__":
    main()
