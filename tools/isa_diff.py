#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    tools/isa_diff.py before.s after.s [--title TEXT]

Prints markdown.  For every kernel of either file: whether the instruction text is identical
(comments, blank lines and the per-file __hip_cuid symbol aside); if not, whether the opcode
sequence is, and then the kernel metadata (.vgpr_count, .sgpr_count, both spill counts,
.private_segment_fixed_size, .group_segment_fixed_size), the instruction counts per class
(v_mfma*, ds_*, global_*, buffer_*, s_waitcnt, s_barrier) before and after, every opcode
whose count differs, and how many of the changed places lie inside the kernel's block loops
(the innermost loops that hold v_mfma instructions; register numbers ignored).  Exit status 1
when a kernel exists in one file only.  A refactor of the hand-scheduled kernels is checked
with it (profiles/ws_share_isa.md)."""
import argparse
import collections
import difflib
import re
import shutil
import subprocess
import sys

META = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size"]
CLASSES = ["v_mfma", "ds_", "global_", "buffer_", "s_waitcnt", "s_barrier"]


def kernels(path):
    """{kernel symbol: (instruction lines, metadata dict)}"""
    text = open(path).read().splitlines()
    meta, cur = {}, None
    for l in text:                                    # the amdhsa.kernels YAML at the end
        s = l.strip()
        if l.startswith("  - ."):                     # a kernel's entry (its .args nest deeper)
            cur = {}
            s = s.lstrip("- ")
        elif s.startswith("- ."):
            continue
        if cur is not None and s.startswith("."):
            k, _, v = s.partition(":")
            v = v.strip()
            if k == ".name":
                meta[v] = cur
            elif k in META:
                cur[k] = int(v)
    body, name, out = [], None, {}
    for l in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in meta and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = (body, meta[name])
            name = None
            continue
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") and not s.endswith(":"):    # directives
            continue
        body.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", s))
    return out


def opcode(line):
    return None if line.endswith(":") else line.split()[0]


def changes_in_mfma_loops(a, b):
    """(changed places inside the innermost loops of `a` that contain MFMAs, all changed places),
    comparing with register numbers masked"""
    lab = {l[:-1]: i for i, l in enumerate(a) if l.endswith(":")}
    loops = [(lab[l.split()[-1]], i) for i, l in enumerate(a)
             if l.startswith("s_cbranch") and lab.get(l.split()[-1], i) < i]
    loops = [lp for lp in loops if any(x.startswith("v_mfma") for x in a[lp[0]:lp[1]])]
    loops = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    mask = lambda l: re.sub(r"\b([vsa])\[?\d+(:\d+)?\]?", r"\1#", l)
    ops = difflib.SequenceMatcher(None, [mask(x) for x in a], [mask(x) for x in b], autojunk=False).get_opcodes()
    ch = [i1 for tag, i1, _, _, _ in ops if tag != "equal"]
    return sum(any(lo <= i <= hi for lo, hi in loops) for i in ch), len(ch)


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool, *names], capture_output=True, text=True, check=True)
        short = [re.sub(r"^void qtx::|\(qtx::RowGemmArgs\)$", "", s) for s in r.stdout.splitlines()]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--title", default=None)
    a = ap.parse_args()
    A, B = kernels(a.before), kernels(a.after)
    names = sorted(set(A) | set(B))
    pretty = demangle(names)
    print(f"### {a.title or a.before + ' -> ' + a.after}\n")
    print("| kernel | instructions | text | opcode sequence |")
    print("|---|---|---|---|")
    details, missing = [], False
    for n in names:
        if n not in A or n not in B:
            print(f"| `{pretty[n]}` | | only in {'before' if n in A else 'after'} | |")
            missing = True
            continue
        (ia, ma), (ib, mb) = A[n], B[n]
        oa = [o for o in map(opcode, ia) if o]
        ob = [o for o in map(opcode, ib) if o]
        same_text, same_ops = ia == ib and ma == mb, oa == ob
        count = f"{len(oa)}" if len(oa) == len(ob) else f"{len(oa)} -> {len(ob)}"
        print(f"| `{pretty[n]}` | {count} | {'identical' if same_text else 'differs'} | "
              f"{'identical' if same_ops else 'differs'} |")
        if not same_text:
            details.append((n, ma, mb, oa, ob, changes_in_mfma_loops(ia, ib)))
    for n, ma, mb, oa, ob, (inl, tot) in details:
        print(f"\n`{pretty[n]}`\n")
        print("| | before | after |")
        print("|---|---|---|")
        for k in META:
            print(f"| `{k}` | {ma.get(k)} | {mb.get(k)} |")
        for c in CLASSES:
            print(f"| `{c}*` | {sum(o.startswith(c) for o in oa)} | {sum(o.startswith(c) for o in ob)} |")
        ca, cb = collections.Counter(oa), collections.Counter(ob)
        diff = [f"`{o}` {ca[o]} -> {cb[o]}" for o in sorted(set(ca) | set(cb)) if ca[o] != cb[o]]
        print("\nopcode counts that differ: " + (", ".join(diff) if diff else "none (registers or order only)"))
        print(f"\nchanged places (register numbers aside): {tot}, of them inside the MFMA block loops: {inl}")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
