#!/usr/bin/env python3
"""live_fir_bench.py -- what an FIR filter per link costs the live medium (afsk_live_mix_filtered, live.LiveMedium with
filters=) against the delayed mix of the same links, and the delayed and the undelayed mix against the parent commit's.

    python tools/live_fir_bench.py [--parent PARENT.so] [--channels 65536] [--reps 3] [--json OUT] [--txt OUT]
    python tools/live_fir_bench.py --step mix2048|mix8192 ...    (one step, in this process)

Without --step the tool is a driver shaped like tools/live_delay_bench.py (whose helpers, and those of
tools/live_mix_bench.py and tools/live_tx_rated_bench.py, it uses): the steps run one after the other, each as a fresh
child process under its own `timeout`, and the chain stops at the first one that fails -- nothing more is started on the
GPU after a fault, an abort or a time limit.  A step compares all its variants in ONE process over the same buffers:
every variant's call is captured once into a HIP graph and replayed, HIP events around each replay give the time, and
the passes take turns.

Workload (n = --channels output rows, T = 2048 or 8192 columns): three unity sources per row at delays (0, 480, 4800),
hist_len 8192, as tools/live_delay_bench.py's `delayed`.
  mix            the undelayed medium: one launch
  delayed        the delayed medium: three launches
  fir1_kK        the filtered medium, the FIRST of the three links through a K-tap filter (K = 1, 16, 64, 256; K = 1 is
                 the identity {16384}, the others fir_design(K, 0, 3000))
  fir3_kK        all three links through it
  parent, parent2            mix from --parent, loaded twice: the difference of the two copies is the spread identical
                 code shows in this run
  parent_delayed             the delayed medium from --parent
The first tick of every variant is checked: the K = 1 variants equal `delayed` bit for bit, the others equal the rule
written out in numpy on three rows.  Every medium lives in its variant's record for as long as the graph that captured
it.  --json / --txt append this run to OUT when it exists."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import live_mix_bench as MB  # noqa: E402
import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native, live  # noqa: E402
from afskmodem_amd.live import LiveMedium  # noqa: E402

SIZES = (2048, 8192)
STEPS = {f"mix{T}": 420 for T in SIZES}
HIST = 8192
DELAYS = (0, 480, 4800)
TAPS = (1, 16, 64, 256)


def taps_of(K):
    return [16384] if K == 1 else live.fir_design(K, 0, 3000)


def rule_rows(src_rows, filtered, K):
    """The first tick's output rows written out in numpy: src_rows [3][rows, T] int16 (the three sources of the checked
    rows), ``filtered``: which of the three links carry the K-tap filter."""
    h = np.asarray(taps_of(K), np.int64)
    acc = 0
    for x, d, f in zip(src_rows, DELAYS, filtered):
        x = x.astype(np.int64)
        late = np.zeros_like(x)
        if d < x.shape[1]:
            late[:, d:] = x[:, : x.shape[1] - d]
        if f:
            v = np.zeros_like(late)
            for i, t in enumerate(h):
                v[:, i:] += t * late[:, : late.shape[1] - i]
            late = np.clip(v >> 14, -32768, 32767)
        acc = acc + late                                        # (unity gain: (32768 * x) >> 15 = x)
    return np.clip(acc, -32768, 32767).astype(np.int16)


def step_mix(torch, libs, n, T, reps, lines, results):
    src = MB.signal(torch, 3 * n, T, 1)
    out = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    delay = dict(delay=[list(DELAYS)], max_delay=HIST)
    plan = [("mix", libs["this"], {}, None), ("delayed", libs["this"], delay, None)]
    for K in TAPS:
        plan.append((f"fir1_k{K}", libs["this"], dict(delay, filters=[taps_of(K)], filter=[[0, None, None]]), (K, (1, 0, 0))))
        plan.append((f"fir3_k{K}", libs["this"], dict(delay, filters=[taps_of(K)], filter=0), (K, (1, 1, 1))))
    if "parent" in libs:
        plan = [("parent", libs["parent"], {}, None), ("parent_delayed", libs["parent"], delay, None)] + plan + \
            [("parent2", libs["parent2"], {}, None)]
    variants = []                                               # (name, lib, graph, the medium the graph reads, check)
    for name, lib, kw, check in plan:
        with B.using(lib):
            m = LiveMedium.from_matrix([[1.0, 1.0]], n, extra=1, **kw)
            assert m.hist_len == (HIST if kw else 0) and bool(getattr(m, "filtered", False)) == ("filters" in kw), name
            variants.append((name, lib, B.capture(torch, lambda side, m=m: m.mix(src, out=out, stream=side)), m, check))
    rows = [0, 1, n - 1]
    host = [src[[r + s * n for r in rows]].cpu().numpy() for s in range(3)]
    firsts = {}
    for name, _, g, m, check in variants:
        if m.delayed:
            m.reset()                                           # (the capture ran nothing; the first replay is tick 0)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        if name in ("mix", "delayed", "parent", "parent_delayed", "parent2"):
            firsts[name] = out.clone()
        elif check[0] == 1:
            assert torch.equal(out, firsts["delayed"]), (name, "differs from the delayed mix")
        else:
            assert np.array_equal(out[rows].cpu().numpy(), rule_rows(host, check[1], check[0])), (name, "differs from the rule")
    for a, b in (("parent", "mix"), ("parent2", "mix"), ("parent_delayed", "delayed")):
        if a in firsts:
            assert torch.equal(firsts[a], firsts[b]), (a, "differs from this build's")
    firsts.clear()
    packed = [(name, lib, None, m, g) for name, lib, g, m, _ in variants]
    us = B.rotate(torch, packed, reps, lambda v: [B.timed(torch, v[4]) for _ in range(MB.REPLAYS)])
    base = B.stats(us["delayed"])
    lines.append(f"{'mix' + str(T):9s} {n}x{T}   delayed {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"{base['samples']} replays)")
    pairs = [("parent2", "parent"), ("mix", "parent"), ("delayed", "parent_delayed")]
    pairs += [(f"fir{w}_k{K}", "delayed") for w in (1, 3) for K in TAPS]
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
        doc = dict(tool="tools/live_fir_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(step=args.step, channels=args.channels, reps=args.reps, parent=bool(args.parent),
                                hist_len=HIST, delays=list(DELAYS), taps=list(TAPS), results=results))
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (its mixes are timed next to this build's)")
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
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
