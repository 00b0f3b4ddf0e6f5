#!/usr/bin/env python3
"""compare_kernel_isa.py -- do two builds of one translation unit hold the same kernels?

    python tools/compare_kernel_isa.py OLD.s NEW.s [--only SUBSTRING]

OLD.s / NEW.s: the device assembly of the unit from two source trees (hipcc with the build's flags and -save-temps
leaves <unit>-hip-amdgcn-amd-amdhsa-gfx950.s).  Per kernel (a symbol whose name holds "kernel"): SAME when every
instruction line and local label is equal (comments and directives dropped), DIFF with the first differing lines, NEW /
GONE when only one side has it.  Exit status 1 when a kernel both sides have differs.  DESIGN.md 8.5 records one use:
the tap's commit against its parent, every existing kernel of afsk_gate.hip SAME."""
import argparse
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip() or (s.strip().startswith(".") and not re.match(r"^\.LBB", s.strip())):
            continue
        out[cur].append(s)
    return {k: v for k, v in out.items() if "kernel" in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    a, b = kernels(args.old), kernels(args.new)
    differ = False
    for k in sorted(set(a) | set(b)):
        if args.only not in k:
            continue
        if k not in a:
            print(f"NEW   {k}  {len(b[k])} lines")
        elif k not in b:
            print(f"GONE  {k}")
        elif a[k] == b[k]:
            print(f"SAME  {k}  {len(a[k])} lines")
        else:
            differ = True
            print(f"DIFF  {k}  {len(a[k])} / {len(b[k])} lines")
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                if x != y:
                    print(f"      line {i}: {x.strip()}  |  {y.strip()}")
                    break
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
