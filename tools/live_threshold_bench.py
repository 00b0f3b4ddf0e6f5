#!/usr/bin/env python3
"""live_threshold_bench.py -- what a threshold pair per channel costs a live receiver's push, in one process.

    python tools/live_threshold_bench.py [--parent PARENT.so] [--shapes 65536x8192,65536x2048] [--seconds 2]
                                         [--reps 6] [--kinds stored,stream] [--variants a,b,...] [--reverse]
                                         [--json OUT] [--txt OUT]

Per shape (channels x T samples per chunk), 1200 baud on every channel, one buffer of synth.live_channels captures
(two bursts of 4 / 12 / 24 bytes, training 0.25 s, every eighth channel silent, 30 dB) pushed by every variant.  A
variant's pushes are captured once, one HIP graph per column window, and replayed; HIP events around each replay give
us per push.  Every round replays the variants one after the other, starting one variant later each round, so that no
variant always runs behind the same neighbour.

Variants (a baseline is never the code under test: it is the PARENT build, --parent, a libafsk_amd.so of the commit
before per-channel thresholds, loaded next to this build's):
  parent, parent2   the parent library, loaded twice (a copy under another name): scalar thresholds.  Their
                    difference is the spread identical code shows in this run -- the control of every comparison.
  scalar, scalar2   this build, scalar thresholds (18000 / 14000), created twice: must be the parent's push; their
                    difference is the same control on this build's code.  The four are created parent, scalar, parent2,
                    scalar2, so that the two copies of a build lie as far apart as the two builds do.
  start_pc          this build, a distinct amp_start per channel (18000 + c % 997), one amp_end: the per-channel gate,
                    one squelch class (the demod launch of `scalar`).
  classes4, classes16   (stored) amp_end 14000 - c % 4 / c % 16: the gate plus one demod launch per class.
  pairs2048         (stream) 2048 distinct pairs (18000 + c % 2048, 14000 - c % 2048).
The thresholds stay within 2048 of the defaults, far from the signal's and the noise's levels, so every variant gates
and decodes the same bursts: the figures compare launches, not workloads.  Without --parent only this build runs.
--reverse creates the variants (their state and output allocations) in the opposite order.
--json / --txt append this run to OUT when it exists (OUT.json: {"tool", "runs": [one record per invocation]}).
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from afskmodem_amd import _native, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver  # noqa: E402

MAX_BURST = 49152            # a 1200-baud burst of 24 bytes is ~30000 samples


class Library:
    """One build of the library, bound like _native.lib().  A build without the per-channel entries (the parent)
    serves the constructor's arrays of one value through its own scalar create entries."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.has_thresholds = hasattr(self.L, "afsk_live_create_thresholds")
        for table in (_native.SIGNATURES, _native.SPLIT_SIGNATURES, _native.LIVE_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                      _native.LIVE_MIXED_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                      _native.LIVE_CLASS_SIGNATURES):
            for name, (res, args) in table.items():
                if hasattr(self.L, name):
                    fn = getattr(self.L, name)
                    fn.restype, fn.argtypes = res, args

    def __getattr__(self, name):
        if not self.has_thresholds and name in _native.LIVE_THRESHOLD_SIGNATURES:
            scalar = self.L.afsk_live_create_mixed if name == "afsk_live_create_thresholds" else self.L.afsk_live_create_stream

            def create(n, bf, start, end, cap, chunk, out):
                s, e = np.ctypeslib.as_array(start, (n,)), np.ctypeslib.as_array(end, (n,))
                assert (s == s[0]).all() and (e == e[0]).all(), "the parent build has scalar thresholds only"
                return scalar(n, bf, int(s[0]), int(e[0]), cap, chunk, out)
            return create
        return getattr(self.L, name)


class using:
    """Route the package's native calls to one Library for the duration."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = _native._lib
        _native._lib = self.lib

    def __exit__(self, *exc):
        _native._lib = self.saved


def thresholds(variant, n):
    c = np.arange(n)
    if variant in ("parent", "parent2", "scalar", "scalar2"):
        return 18000, 14000
    if variant == "start_pc":
        return 18000 + c % 997, 14000
    if variant.startswith("classes"):
        return 18000 + c % 997, 14000 - c % int(variant[7:])
    if variant == "pairs2048":
        return 18000 + c % 2048, 14000 - c % 2048
    raise ValueError(variant)


class Variant:
    def __init__(self, torch, name, kind, lib, data, T):
        self.name, self.lib = name, lib
        n, total = data.shape
        start, end = thresholds(name, n)
        as_arg = lambda v: v if np.ndim(v) == 0 else v.tolist()  # noqa: E731
        with using(lib):
            self.rx = LiveReceiver(n, 40, as_arg(start), as_arg(end), max_burst_len=MAX_BURST if kind == "stored" else None,
                                   max_chunk_len=T)
            self.outs = [self.rx.alloc_result() for _ in range(2)]
            self.graphs = []
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for p in range(total // T):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=side):
                        self.rx.push(data[:, p * T: (p + 1) * T], out=self.outs[p % 2])
                    self.graphs.append(g)
            torch.cuda.synchronize()
        self.us = []
        self.decoded = None

    def replay(self, torch, keep):
        with using(self.lib):
            self.rx.flush()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in self.graphs]
        decoded = 0
        for g, (a, b) in zip(self.graphs, ev):
            a.record()
            g.replay()
            b.record()
        torch.cuda.synchronize()
        if keep:
            self.us += [a.elapsed_time(b) * 1e3 for a, b in ev]
        else:                                   # the warm-up round also counts what a variant decodes
            with using(self.lib):
                self.rx.flush()
            for p, g in enumerate(self.graphs):
                g.replay()
                decoded += int((self.outs[p % 2].demod.nbytes > 0).sum())
            self.decoded = decoded

    def close(self, torch):
        torch.cuda.synchronize()
        del self.graphs
        with using(self.lib):
            self.rx.close()


def stats(us):
    us = np.asarray(us)
    return dict(us_mean=round(float(us.mean()), 2), us_median=round(float(np.median(us)), 2),
                us_p90=round(float(np.percentile(us, 90)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit")
    ap.add_argument("--shapes", default="65536x8192,65536x2048")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--kinds", default="stored,stream")
    ap.add_argument("--variants", default="")
    ap.add_argument("--reverse", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    import torch
    _native.require_device()
    this = Library(_native.LIB_PATH)
    libs = {"this": this}
    tmp = None
    if args.parent:
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = Library(args.parent), Library(twin)
    results, lines = [], []
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        total = int(args.seconds * 48000) // T * T
        data, _ = synth.live_channels(n, total, 1200, args.seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                      silent_every=8, device="cuda")
        for kind in args.kinds.split(","):
            names = (["parent", "scalar", "parent2"] if args.parent else ["scalar"]) + ["scalar2", "start_pc"]
            names += ["classes4", "classes16"] if kind == "stored" else ["pairs2048"]
            if args.variants:
                names = [v for v in names if v in args.variants.split(",")]
            if args.reverse:
                names = names[::-1]
            vs = [Variant(torch, v, kind, libs.get(v, this), data, T) for v in names]
            for r in range(args.reps + 1):
                for i in range(len(vs)):
                    vs[(i + r) % len(vs)].replay(torch, keep=r > 0)
            recs = {}
            for v in vs:
                recs[v.name] = dict(kind=kind, shape=shape, variant=v.name, pushes=len(v.us), launches_per_push=(
                    1 if kind == "stream" else 1 + max(1, len(set(np.atleast_1d(thresholds(v.name, n)[1]).tolist())))),
                    state_bytes=v.rx.state_bytes, slots_decoded=v.decoded, **stats(v.us))
                print(json.dumps(recs[v.name]), flush=True)
                v.close(torch)
            results += list(recs.values())
            assert len({r["slots_decoded"] for r in recs.values()}) == 1, "the variants decode different bursts"
            base = recs.get("parent")
            if base and "parent2" in recs:
                spread = abs(recs["parent2"]["us_mean"] / base["us_mean"] - 1.0)
                lines.append(f"{kind:7s} {shape:11s} parent {base['us_mean']:7.1f} / {base['us_median']:7.1f} us (mean / median)"
                             f"   parent2 {recs['parent2']['us_mean']:7.1f} / {recs['parent2']['us_median']:7.1f}"
                             f"   spread {100 * spread:.2f} %")
                if "scalar" in recs and "scalar2" in recs:
                    own = abs(recs["scalar2"]["us_mean"] / recs["scalar"]["us_mean"] - 1.0)
                    lines[-1] += f"   (scalar2 against scalar {100 * own:.2f} %)"
                for name, r in recs.items():
                    if name in ("parent", "parent2"):
                        continue
                    ratio = r["us_mean"] / base["us_mean"]
                    cmp_ = dict(kind=kind, shape=shape, variant=name, over_parent_mean=round(ratio, 4),
                                over_parent_median=round(r["us_median"] / base["us_median"], 4),
                                parent_spread=round(spread, 4), inside_spread=bool(abs(ratio - 1.0) <= spread))
                    results.append(cmp_)
                    print(json.dumps(cmp_), flush=True)
                    lines.append(f"{'':7s} {'':11s} {name:10s} {r['us_mean']:7.1f} / {r['us_median']:7.1f} us   x{ratio:.3f} of parent"
                                 f" (median x{cmp_['over_parent_median']:.3f})   {r['launches_per_push']} launches"
                                 f"   {'inside' if cmp_['inside_spread'] else 'OUTSIDE'} the spread")
            torch.cuda.empty_cache()
        del data
        torch.cuda.empty_cache()
    if args.json:
        doc = dict(tool="tools/live_threshold_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(seconds=args.seconds, reps=args.reps, reverse=args.reverse, shapes=args.shapes,
                                kinds=args.kinds, variants=args.variants, results=results))
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
    if args.txt:
        with open(args.txt, "a") as f:
            f.write(f"run{' --reverse' if args.reverse else ''}\n" + "\n".join(lines) + "\n\n")
    if tmp:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
