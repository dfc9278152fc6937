"""Compare the kernels of two device-assembly files (hipcc --cuda-device-only -S of the same
source before and after a change): per kernel the instruction stream with branch labels
normalised and the code object notes' register counts, LDS and scratch sizes.

Usage: python tools/asm_identity.py before.s after.s [title] > profiles/NAME_kernels.txt
"""
from __future__ import annotations

import re
import subprocess
import sys

NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    txt = open(path).read()
    notes = {}
    for blk in re.split(r"\n  - \.agpr_count:", "\n" + txt.split("amdhsa.kernels:")[-1])[1:]:
        blk = "  - .agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        notes[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in NOTES)
    body = {}
    for name in notes:
        m = re.search(r"^%s:.*?\n(.*?)^\s*\.section\s+\.rodata" % re.escape(name), txt, re.S | re.M)
        lines = []
        labels = {}
        for ln in m.group(1).split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                lab = re.match(r"(\.LBB\d+_\d+):", ln)
                if lab:
                    labels[lab.group(1)] = "L%d" % len(labels)
                    lines.append(lab.group(1) + ":")
                continue
            lines.append(ln)
        s = "\n".join(lines)
        s = re.sub(r"\.LBB\d+_\d+", lambda q: labels.get(q.group(0), "L?"), s)
        body[name] = s
    return notes, body


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(set(before[0]) | set(after[0])))
    # a template parameter appended with its default value changes the mangled name only
    b = {names[n]: n for n in before[0]}
    a = {}
    for n in after[0]:
        short = re.sub(r", false>\(", ">(", names[n], count=1)
        a[short if names[n] not in b and short in b else names[n]] = n
    same = [k for k in b if k in a and before[0][b[k]] == after[0][a[k]] and before[1][b[k]] == after[1][a[k]]]
    if len(sys.argv) > 3:
        print(sys.argv[3])
    print(f"{len(b)} kernels before, {len(a)} after; identical (instruction stream with labels normalised, "
          f"VGPR/AGPR/SGPR counts, LDS, scratch): {len(same)} of {len(b)}")
    for k in sorted(a):
        n = after[0][a[k]]
        tag = "new " if k not in b else ("same" if k in same else "DIFF")
        print(f"{tag} {k[:100]:100s} instr {after[1][a[k]].count(chr(10)) + 1:6d} vgpr {n[0]:3d} agpr {n[1]:3d} "
              f"sgpr {n[2]:3d} lds {n[3]:6d} scratch {n[4]}")
    return 0 if len(same) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main())
