#!/usr/bin/env python3
"""live_delay_bench.py -- what a delay per link costs the live medium (afsk_live_mix_delayed, live.LiveMedium with
delays) against the undelayed mix of the same build and of the parent commit.

    python tools/live_delay_bench.py [--parent PARENT.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_delay_bench.py --step mix2048|mix8192 ...    (one step, in this process)

Without --step the tool is a driver shaped like tools/live_mix_bench.py (whose signal, and the helpers of
tools/live_tx_rated_bench.py, it uses): the steps run one after the other, each as a fresh child process under its own
`timeout`, and the chain stops at the first one that fails -- nothing more is started on the GPU after a fault, an abort
or a time limit.  A step compares all its variants in ONE process over the same buffers: every variant's call is
captured once into a HIP graph and replayed, HIP events around each replay give the time, and the passes take turns.

Workload (n = --channels output rows, T = 2048 or 8192 columns): three unity sources per row (station A | station B | a
third sender, as LiveMedium.from_matrix([[1, 1]], n, extra=1) lays them out).
  mix        medium.mix(src, out=out) of the undelayed medium: one launch
  delayed0   the delayed medium (hist_len 8192) with every delay 0: three launches, the output checked equal to mix's
  delayed    the delayed medium with delays (0, 480, 4800) samples at hist_len 8192, its first tick checked against the
             torch expression over shifted rows
  parent, parent2   mix from --parent, loaded twice: the difference of the two copies is the spread identical code
             shows in this run
Every medium lives in its variant's record for as long as the graph that captured it: the graph reads its tables, its
position and its history.  --json / --txt append this run to OUT when it exists."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import live_mix_bench as MB  # noqa: E402
import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native  # noqa: E402
from afskmodem_amd.live import LiveMedium  # noqa: E402

SIZES = (2048, 8192)
STEPS = {f"mix{T}": 300 for T in SIZES}
HIST = 8192
DELAYS = (0, 480, 4800)


def shifted(torch, x, d):
    """x delayed by d columns, zeros in front: what a medium that has sent nothing yet hears in its first tick."""
    if d == 0:
        return x
    out = torch.zeros_like(x)
    if d < x.shape[1]:
        out[:, d:] = x[:, : x.shape[1] - d]
    return out


def step_mix(torch, libs, n, T, reps, lines, results):
    src = MB.signal(torch, 3 * n, T, 1)
    out = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    parts = (src[:n], src[n: 2 * n], src[2 * n:])
    plan = [("mix", libs["this"], None), ("delayed0", libs["this"], (0, 0, 0)), ("delayed", libs["this"], DELAYS)]
    if "parent" in libs:
        plan = [("parent", libs["parent"], None)] + plan + [("parent2", libs["parent2"], None)]
    variants = []                                               # (name, lib, graph, the medium the graph reads)
    for name, lib, delays in plan:
        with B.using(lib):
            kw = {} if delays is None else dict(delay=[list(delays)], max_delay=HIST)
            m = LiveMedium.from_matrix([[1.0, 1.0]], n, extra=1, **kw)
            assert (delays is not None) == bool(getattr(m, "delayed", False)), name
            if delays is not None:
                assert m.hist_len == HIST
            variants.append((name, lib, B.capture(torch, lambda side, m=m: m.mix(src, out=out, stream=side)), m))
    want = torch.zeros_like(out)
    MB.torch_medium(torch, want, parts)
    assert int((want == 32767).sum()) > 0 and int((want == -32768).sum()) > 0, "nothing clips"
    late = torch.zeros_like(out)
    MB.torch_medium(torch, late, tuple(shifted(torch, p, d) for p, d in zip(parts, DELAYS)))
    for name, _, g, m in variants:
        if name.startswith("delayed"):
            m.reset()                                           # (the capture ran nothing; the first replay is tick 0)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, late if name == "delayed" else want), (name, "differs from the torch expression")
    del want, late
    packed = [(name, lib, None, m, g) for name, lib, g, m in variants]
    us = B.rotate(torch, packed, reps, lambda v: [B.timed(torch, v[4]) for _ in range(MB.REPLAYS)])
    base = B.stats(us["mix"])
    lines.append(f"{'mix' + str(T):9s} {n}x{T}   mix {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"{base['samples']} replays)")
    pairs = [("parent2", "parent"), ("mix", "parent"), ("delayed0", "mix"), ("delayed", "mix"), ("delayed", "delayed0")]
    B.report(f"mix{T}", f"{n}x{T}", us, pairs, lines, results)
    torch.cuda.synchronize()
    while packed:                                               # the graphs go before the media they read
        name, lib, _, m, g = packed.pop()
        del g
    del variants[:]


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": B.Library(_native.LIB_PATH)}
    T = int(args.step[len("mix"):])
    tmp = None
    if args.parent:
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = B.Library(args.parent), B.Library(twin)
    lines, results = [], []
    step_mix(torch, libs, args.channels, T, args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_delay_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(step=args.step, channels=args.channels, reps=args.reps, parent=bool(args.parent),
                                hist_len=HIST, delays=list(DELAYS), results=results))
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
    if args.txt:
        with open(args.txt, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    print("\n".join(lines))
    if tmp:
        shutil.rmtree(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (its mix is timed next to this build's)")
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--steps", help="comma-separated steps for the driver (default: all)")
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    # the driver: every step a fresh process under its own time limit, the chain ends at the first failure
    for step in (args.steps.split(",") if args.steps else STEPS):
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--channels", str(args.channels), "--reps", str(args.reps)]
        for flag in ("parent", "json", "txt"):
            if getattr(args, flag):
                cmd += ["--" + flag, getattr(args, flag)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is run", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
