#!/usr/bin/env python3
"""live_level_bench.py -- what the level tracker (LiveReceiver(..., level=True), afsk_live_level) costs in front of the
streaming receiver's push, and whether the fixed push of this build is still the parent's.

    python tools/live_level_bench.py [--shapes 65536x2048,65536x8192] [--seconds 2] [--reps 3] [--parent PARENT.so]
                                     [--other OTHER.so] [--json OUT] [--txt OUT]

Per shape (channels x T samples per push): tools/live_bench.py's 1200-baud workload (two bursts per channel with
payloads of 4 / 12 / 24 bytes at random leads, every eighth channel silent, noise at 30 dB).  Every push is a column
window of that buffer, captured once into a graph per window position and replayed with device events around each
replay; the variants take turns pass by pass after one warm-up pass each (tools/live_bench.py's timed_pass), so drift
hits all alike:
  parent, parent_again   with --parent (a libafsk_amd.so of the parent commit): that build's fixed streaming push,
                         twice -- the spread of the repeat is the margin this build's fixed push has to stay inside
  fixed                  this build's streaming push without level= (the parent's kernels)
  leveled                this build's push with level=True: live_level_kernel + the PER_CHANNEL push, one graph
  tracker                live_level_kernel alone over the same windows (the receiver's state does not move)
  leveled_other, tracker_other   with --other (another build of THIS commit, e.g. build.sh -DAFSK_LIVE_LEVEL_NT=0: the
                         tracker's chunk loads cacheable instead of nontemporal): the same two on that build
Reported per variant: the mean us per push and its ratio to `fixed`; for the tracker also the chunk bytes it reads per
second.  An eager pass counts the payloads the fixed and the leveled receiver decode out of those sent."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from afskmodem_amd import _native, batch, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver  # noqa: E402
from live_bench import BAUD, BF, graphs_for, load_build, timed_pass, using  # noqa: E402


class TrackerOnly:
    """A leveled receiver whose `push` launches the tracker alone: what graphs_for captures and timed_pass replays."""

    def __init__(self, rx):
        self.rx = rx

    def push(self, chunk, out=None):
        rx = self.rx
        _native.check(_native.lib().afsk_live_level(
            rx.handle, rx.level_state.data_ptr(), rx.level_spec.native(), chunk.data_ptr(), int(chunk.stride(0)),
            int(chunk.shape[1]), None, None, batch._stream_ptr(None, rx.device)))

    def flush(self):
        self.rx.flush()

    def close(self):
        self.rx.close()


def timed_variants(torch, samples, n_push, T, reps, parent, other):
    """Every variant's per-window times over `reps` passes: {name: [reps, n_push] us}."""
    n = samples.shape[0]
    variants = ([("parent", parent, None, False), ("parent_again", parent, None, False)] if parent is not None else []) \
        + [("fixed", None, None, False), ("leveled", None, True, False), ("tracker", None, True, True)] \
        + ([("leveled_other", other, True, False), ("tracker_other", other, True, True)] if other is not None else [])
    runs = []
    for name, lib, level, alone in variants:
        with using(lib):
            kw = dict(level=level) if level else {}
            rx = LiveReceiver(n, BF, max_burst_len=None, max_payload_len=256, max_chunk_len=T, **kw)
            if alone:
                rx = TrackerOnly(rx)
            out = None if alone else rx.alloc_result()
            graphs = graphs_for(torch, rx, samples, n_push, T, out)
        runs.append(dict(name=name, lib=lib, rx=rx, graphs=graphs, out=out, passes=[]))
    for r in range(reps + 1):
        for v in runs:
            with using(v["lib"]):
                t = timed_pass(torch, v["rx"], v["graphs"])
            if r:
                v["passes"].append(t)
    torch.cuda.synchronize()
    times = {v["name"]: np.asarray(v["passes"]) for v in runs}
    for v in runs:
        del v["graphs"], v["out"]
        with using(v["lib"]):
            v["rx"].close()
    return times


def cells(times, chunk_bytes):
    out = {}
    for name, t in times.items():
        per_pass = t.mean(axis=1)
        out[name] = dict(us_mean=round(float(t.mean()), 2), us_passes=[round(float(x), 2) for x in per_pass],
                         spread=round(float((per_pass.max() - per_pass.min()) / per_pass.mean()), 4))
        if name.startswith("tracker"):
            out[name]["chunk_tb_per_s"] = round(chunk_bytes / (float(t.mean()) * 1e-6) / 1e12, 3)
    for name, c in out.items():
        c["over_fixed"] = round(c["us_mean"] / out["fixed"]["us_mean"], 4)
    if "parent" in out:
        a, b = out["parent"]["us_mean"], out["parent_again"]["us_mean"]
        margin = max(abs(a - b) / min(a, b), out["parent"]["spread"], out["parent_again"]["spread"])
        out["margin"] = round(margin, 4)
        out["fixed_over_parent"] = round(out["fixed"]["us_mean"] / (0.5 * (a + b)), 4)
        out["fixed_inside_margin"] = bool(out["fixed"]["us_mean"] <= max(a, b) * (1 + margin))
    return out


def decoded(torch, samples, sent, n_push, T, level):
    """An eager pass: how many of the payloads sent the receiver returns."""
    n = samples.shape[0]
    rx = LiveReceiver(n, BF, max_burst_len=None, max_payload_len=256, max_chunk_len=T, level=level)
    out, ev = rx.alloc_result(), rx.alloc_events()
    got = [[] for _ in range(n)]
    for p in range(n_push):
        res = rx.push(samples[:, p * T: (p + 1) * T], out=out, flush=p == n_push - 1, events=ev)
        for c, _, _, payload in res.events.bursts():
            got[c].append(payload)
    rx.close()
    return sum(sum(1 for _, b in sent[c] if b in got[c]) for c in range(n))


def run_shape(torch, n, T, seconds, reps, seed, parent, other):
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    samples, sent = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                        silent_every=8, device="cuda")
    rec = dict(shape=f"{n}x{T}", baud=BAUD, pushes=n_push, reps=reps, bursts_sent=sum(len(s) for s in sent),
               decoded_fixed=decoded(torch, samples, sent, n_push, T, None),
               decoded_leveled=decoded(torch, samples, sent, n_push, T, True),
               workload=cells(timed_variants(torch, samples, n_push, T, reps, parent, other), 2 * n * T))
    del samples
    torch.cuda.empty_cache()
    return rec


def lines_of(rec):
    out = [f"{rec['shape']} @{rec['baud']}  {rec['pushes']} pushes per pass, {rec['reps']} passes; payloads returned "
           f"(eager): fixed {rec['decoded_fixed']}/{rec['bursts_sent']}, leveled {rec['decoded_leveled']}/{rec['bursts_sent']}"]
    c = rec["workload"]
    out.append("  us per push, mean (x fixed)")
    for name in ("parent", "parent_again", "fixed", "leveled", "tracker", "leveled_other", "tracker_other"):
        if name in c:
            v = c[name]
            rate = f"   chunk read at {v['chunk_tb_per_s']:.2f} TB/s" if "chunk_tb_per_s" in v else ""
            out.append(f"    {name:14s} {v['us_mean']:10.1f} x{v['over_fixed']:.4f} (spread {100 * v['spread']:.2f} %){rate}")
    if "margin" in c:
        out.append(f"    fixed/parent x{c['fixed_over_parent']:.4f} (margin {100 * c['margin']:.2f} %: "
                   f"{'inside' if c['fixed_inside_margin'] else 'OUTSIDE'})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x2048,65536x8192")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit: its fixed streaming push, timed in the same run")
    ap.add_argument("--other", help="another build of this commit (e.g. -DAFSK_LIVE_LEVEL_NT=0): its leveled push and tracker")
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    import torch
    parent = load_build(args.parent) if args.parent else None
    other = load_build(args.other) if args.other else None
    res, lines = [], []
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        rec = run_shape(torch, n, T, args.seconds, args.reps, args.seed, parent, other)
        print(json.dumps(rec), flush=True)
        res.append(rec)
        lines += lines_of(rec)
    print("\n".join(lines))
    for path, text in ((args.json, json.dumps(dict(tool="tools/live_level_bench.py", parent=bool(args.parent),
                                                   other=bool(args.other), seconds=args.seconds, reps=args.reps,
                                                   results=res), indent=1)),
                       (args.txt, "\n".join(lines) + "\n")):
        if path:
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
