#!/usr/bin/env python3
"""compare_kernel_isa.py -- do two builds of one translation unit hold the same kernels?

    python tools/compare_kernel_isa.py OLD.s NEW.s [--only SUBSTRING] [--map OLD_SUBSTRING=NEW_SUBSTRING ...]

OLD.s / NEW.s: the device assembly of the unit from two source trees (hipcc with the build's flags and -save-temps
leaves <unit>-hip-amdgcn-amd-amdhsa-gfx950.s).  Per kernel (a symbol whose name holds "kernel"): SAME when every
instruction line and local label is equal (comments and directives dropped, the function's number in .LBB labels
ignored), DIFF with the first differing lines, NEW / GONE when only one side has it.  Exit status 1 when a kernel both
sides have differs.  DESIGN.md 8.5 records one use: the tap's commit against its parent, every existing kernel of
afsk_gate.hip SAME.

--map (repeatable) pairs a renamed kernel with its twin: the one old kernel whose name holds OLD_SUBSTRING with the one
new kernel whose name holds NEW_SUBSTRING.  A pair is printed as PAIR (SAME / DIFF as above) with both names and, per
side, the instruction lines and the kernel's SGPRs, VGPRs, LDS bytes and scratch bytes from its "Kernel info" comment;
a differing pair does not change the exit status (the twelve gate kernels against live_push_kernel's
cells)."""
import argparse
import re
import sys

INFO = (("sgpr", r"; TotalNumSgprs: (\d+)"), ("vgpr", r"; TotalNumVgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
        ("scratch", r"; ScratchSize: (\d+)"))


def kernels(path):
    """{name: (instruction lines, {sgpr, vgpr, lds, scratch})}"""
    out, info, cur, last = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = last = m.group(1)
            out[cur], info[cur] = [], {}
            continue
        if cur is None:
            if last is not None and line.startswith(";"):
                for key, pat in INFO:
                    m = re.match(pat, line)
                    if m:
                        info[last].setdefault(key, int(m.group(1)))
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip() or (s.strip().startswith(".") and not re.match(r"^\.LBB", s.strip())):
            continue
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {k: (v, info[k]) for k, v in out.items() if "kernel" in k}


def figures(k):
    lines, info = k
    return f"{len(lines)} lines, " + ", ".join(f"{key} {info.get(key, '?')}" for key, _ in INFO)


def first_difference(x, y):
    for i, (p, q) in enumerate(zip(x, y)):
        if p != q:
            return f"      line {i}: {p.strip()}  |  {q.strip()}"
    return f"      line {min(len(x), len(y))}: one side ends"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default="")
    ap.add_argument("--map", action="append", default=[], metavar="OLD_SUBSTRING=NEW_SUBSTRING")
    args = ap.parse_args()
    a, b = kernels(args.old), kernels(args.new)
    paired = {}
    for spec in args.map:
        old, _, new = spec.partition("=")
        ka, kb = [k for k in a if old in k], [k for k in b if new in k]
        if len(ka) != 1 or len(kb) != 1:
            sys.exit(f"--map {spec}: {len(ka)} old and {len(kb)} new kernels match, one of each is needed")
        paired[ka[0]] = kb[0]
    differ = False
    for k in sorted(set(a) | set(b)):
        if args.only not in k or k in paired.values():
            continue
        if k in paired:
            n = paired[k]
            same = a[k][0] == b[n][0]
            print(f"PAIR  {'SAME' if same else 'DIFF'}\n      old {k}\n          {figures(a[k])}\n      new {n}\n"
                  f"          {figures(b[n])}")
            if not same:
                print(first_difference(a[k][0], b[n][0]))
        elif k not in a:
            print(f"NEW   {k}  {len(b[k][0])} lines")
        elif k not in b:
            print(f"GONE  {k}")
        elif a[k][0] == b[k][0]:
            print(f"SAME  {k}  {len(a[k][0])} lines")
        else:
            differ = True
            print(f"DIFF  {k}  {len(a[k][0])} / {len(b[k][0])} lines")
            print(first_difference(a[k][0], b[k][0]))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
