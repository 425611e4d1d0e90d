#!/usr/bin/env python
"""Which kernels of two builds of one source have the same instructions:

    python tools/asm_kernels_diff.py PARENT.s BRANCH.s > profiles/rNN/asm_parent_vs_branch_NAME.txt

Both files come from `hipcc <the library's flags> -S --cuda-device-only FILE.hip` (no GPU needed).  A kernel's text is what
lies between its label and its end label, without comments, directives and blank lines, with the numbers of local labels and of
compiler-made symbols taken out.  One line per kernel: "same" or "differs", and the number of instruction lines on each side."""
import re
import subprocess
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        if re.match(r"^\s+\.", line):                     # a directive
            continue
        cur.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", re.sub(r"__unnamed_\d+", "__unnamed", line.strip())))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in sorted(set(a) | set(b)):
        name = subprocess.run(["c++filt", k], stdout=subprocess.PIPE).stdout.decode().strip()
        name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "").replace("pinn::", "")
        print("%-28s %-8s %6d %6d lines" % (name, "same" if a.get(k) == b.get(k) else "differs", len(a.get(k, [])), len(b.get(k, []))))


if __name__ == "__main__":
    main()
