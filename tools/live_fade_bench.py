#!/usr/bin/env python3
"""live_fade_bench.py -- what a fade track per link costs the live medium (afsk_live_mix_faded, live.LiveMedium with
fades=) against the delayed and the filtered mix of the same links, and the undelayed, the delayed and the filtered mix
against the parent commit's.

    python tools/live_fade_bench.py [--parent PARENT.so] [--channels 65536] [--reps 3] [--json OUT] [--txt OUT]
    python tools/live_fade_bench.py --step mix2048|mix8192 ...    (one step, in this process)

Without --step the tool is a driver shaped like tools/live_fir_bench.py (whose helpers, and those of
tools/live_mix_bench.py and tools/live_tx_rated_bench.py, it uses): the steps run one after the other, each as a fresh
child process under its own `timeout`, and the chain stops at the first one that fails -- nothing more is started on the
GPU after a fault, an abort or a time limit.  A step compares all its variants in ONE process over the same buffers:
every variant's call is captured once into a HIP graph and replayed, HIP events around each replay give the time, and
the passes take turns.

Workload (n = --channels output rows, T = 2048 or 8192 columns): three unity sources per row at delays (0, 480, 4800),
hist_len 8192, as tools/live_fir_bench.py's.  The filter is fir_design(64, 0, 3000), the track
fade_design(256, 1024, 2.0) with fade_offset="spread".
  mix, delayed   the undelayed medium (one launch) and the delayed medium (three launches)
  fir0           the filtered medium with no link through a filter: live_mix_fir_kernel doing the delayed mix's work
  fir1, fir3     the filtered medium: the FIRST of the three links, or all three, through the 64-tap filter
  fade0          the faded medium with no link on a track: live_mix_fade_kernel doing the delayed mix's work
  fade1, fade3   the faded medium: the first link, or all three, along the track; no filter
  fade1_fir, fade3_fir   the same links along the track AND through the filter
  parent, parent2                  mix from --parent, loaded twice: the difference of the two copies is the spread
                                   identical code shows in this run
  parent_delayed, parent_fir1      the delayed and the filtered medium (fir1's) from --parent
The first tick of every variant is checked: this build's mix, delayed and fir1 equal the parent's bit for bit, the others
equal the rule written out in numpy on three rows.  Every medium lives in its variant's record for as long as the graph
that captured it.  --json / --txt append this run to OUT when it exists."""
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
TAPS = 64
TRACK = (256, 1024, 2.0)


def rule_rows(src_rows, rows, filtered, faded, knots, shift):
    """The first tick's output rows written out in numpy: src_rows [3][len(rows), T] int16 (the three sources of the
    checked output rows ``rows``), ``filtered`` / ``faded``: which of the three links carry the filter / the track."""
    h = np.asarray(live.fir_design(TAPS, 0, 3000), np.int64)
    kn = np.asarray(knots, np.int64)
    L, T = kn.size, src_rows[0].shape[1]
    acc = 0
    for s, (x, d) in enumerate(zip(src_rows, DELAYS)):
        x = x.astype(np.int64)
        late = np.zeros_like(x)
        if d < T:
            late[:, d:] = x[:, : T - d]
        if filtered[s]:
            v = np.zeros_like(late)
            for i, t in enumerate(h):
                v[:, i:] += t * late[:, : T - i]
            late = np.clip(v >> 14, -32768, 32767)
        if faded[s]:
            k = np.asarray(rows, np.int64)[:, None] * 3 + s      # the link's CSR index: three links per row
            u = (np.arange(T, dtype=np.int64)[None, :] + k * live.MEDIUM_FADE_SPREAD) & 0xFFFFFFFF
            n = (u >> shift) & (L - 1)
            e = kn[n] + (((kn[(n + 1) & (L - 1)] - kn[n]) * (u & ((1 << shift) - 1))) >> shift)
            late = np.clip((e * late) >> 15, -32768, 32767)
        acc = acc + late                                        # (unity gain: (32768 * x) >> 15 = x)
    return np.clip(acc, -32768, 32767).astype(np.int16)


def step_mix(torch, libs, n, T, reps, lines, results):
    src = MB.signal(torch, 3 * n, T, 1)
    out = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    delay = dict(delay=[list(DELAYS)], max_delay=HIST)
    filt = dict(delay, filters=[live.fir_design(TAPS, 0, 3000)])
    knots, period = live.fade_design(*TRACK)
    fade = dict(fades=[(knots, period)], fade_offset="spread")
    one, all3, none = [[0, None, None]], 0, (0, 0, 0)
    this = libs["this"]
    plan = [("mix", this, {}, None), ("delayed", this, delay, None),
            ("fir0", this, dict(filt, filter=[[None, None, None]]), (none, none)),
            ("fir1", this, dict(filt, filter=one), ((1, 0, 0), none)),
            ("fir3", this, dict(filt, filter=all3), ((1, 1, 1), none)),
            ("fade0", this, dict(delay, **fade, fade=[[None, None, None]]), (none, none)),
            ("fade1", this, dict(delay, **fade, fade=one), (none, (1, 0, 0))),
            ("fade3", this, dict(delay, **fade, fade=all3), (none, (1, 1, 1))),
            ("fade1_fir", this, dict(filt, **fade, filter=one, fade=one), ((1, 0, 0), (1, 0, 0))),
            ("fade3_fir", this, dict(filt, **fade, filter=all3, fade=all3), ((1, 1, 1), (1, 1, 1)))]
    if "parent" in libs:
        plan = [("parent", libs["parent"], {}, None), ("parent_delayed", libs["parent"], delay, None),
                ("parent_fir1", libs["parent"], dict(filt, filter=one), None)] + plan + \
            [("parent2", libs["parent2"], {}, None)]
    variants = []                                               # (name, lib, graph, the medium the graph reads, check)
    for name, lib, kw, check in plan:
        with B.using(lib):
            m = LiveMedium.from_matrix([[1.0, 1.0]], n, extra=1, **kw)
            assert m.hist_len == (HIST if kw else 0) and m.filtered == ("filters" in kw) and m.faded == ("fades" in kw), name
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
        if check is None:
            firsts[name] = out.clone()
        else:
            want = rule_rows(host, rows, check[0], check[1], knots, period.bit_length() - 1)
            assert np.array_equal(out[rows].cpu().numpy(), want), (name, "differs from the rule")
            if name == "fir1":
                firsts[name] = out.clone()
    for a, b in (("parent", "mix"), ("parent2", "mix"), ("parent_delayed", "delayed"), ("parent_fir1", "fir1")):
        if a in firsts:
            assert torch.equal(firsts[a], firsts[b]), (a, "differs from this build's")
    firsts.clear()
    packed = [(name, lib, None, m, g) for name, lib, g, m, _ in variants]
    us = B.rotate(torch, packed, reps, lambda v: [B.timed(torch, v[4]) for _ in range(MB.REPLAYS)])
    base = B.stats(us["delayed"])
    lines.append(f"{'mix' + str(T):9s} {n}x{T}   delayed {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"{base['samples']} replays)")
    pairs = [("parent2", "parent"), ("mix", "parent"), ("delayed", "parent_delayed"), ("fir1", "parent_fir1"),
             ("fir0", "delayed"), ("fir1", "delayed"), ("fir3", "delayed"), ("fade0", "delayed"), ("fade0", "fir0"), ("fade1", "fade0"), ("fade3", "fade0"),
             ("fade1", "delayed"), ("fade3", "delayed"),
             ("fade1_fir", "delayed"), ("fade3_fir", "delayed"), ("fade1_fir", "fir1"), ("fade3_fir", "fir3")]
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
        doc = dict(tool="tools/live_fade_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(step=args.step, channels=args.channels, reps=args.reps, parent=bool(args.parent),
                                hist_len=HIST, delays=list(DELAYS), taps=TAPS, track=list(TRACK), results=results))
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
