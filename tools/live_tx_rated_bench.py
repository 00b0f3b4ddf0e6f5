#!/usr/bin/env python3
"""live_tx_rated_bench.py -- what a rate per queued message costs the live transmitter, measured step by step.

    python tools/live_tx_rated_bench.py [--parent PARENT.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_tx_rated_bench.py --step pull2048|pull8192|submit|relay ...      (one step, in this process)

Without --step the tool is a driver: it runs the four steps one after the other, each as a fresh child process under
its own `timeout`, and stops at the first one that fails -- nothing more is started on the GPU after a fault, an abort
or a time limit.  A step compares all its variants in ONE process over the same buffers: every variant's call is
captured once into a HIP graph and replayed, HIP events around each replay give the time, and the passes take turns
(every pass starts one variant later), so that no variant always runs behind the same neighbour.

The workload is tools/live_bench.py's: 1200 baud, training 0.5 s, payloads of 24 bytes, every channel busy.  Before
each pass a variant's queues are refilled (reset + a submit of queue_depth messages per channel, untimed), and a pass
replays only as many pulls as the shortest queue covers, so no channel idles in a timed pull.

Variants (a baseline is never the code under test: --parent names a libafsk_amd.so of the parent commit, loaded twice
-- the second time as a copy under another name -- and the difference of the two copies is the spread identical code
shows in this run, the yardstick of every comparison against the parent):
  pull     parent / parent2 / uniform   LiveTransmitter(n, 1200)                  of the parent (twice) and of this build
           parent_mixed / parent_mixed2 / mixed   300 / 1200 / 2400 baud on channel c % 3, likewise (in the mixed table
                                        of the report the two parent copies are again named parent and parent2)
           rated1                       a one-entry table [1200]                  against uniform
           rated3_fixed                 table 300 / 1200 / 2400, channel c always at entry c % 3   against mixed
           rated3_rotating              the same table, message m of channel c at entry (c + m) % 3
  submit   parent / parent2 / submit    afsk_live_tx_submit, one message per channel
           submit_rated                 afsk_live_tx_submit_rated with a rate_index array, a one-entry table
  relay    parent / parent2 / events    afsk_live_tx_submit_events of a packed list in which 64 or all channels closed
                                        a burst of 16 bytes
           events_heard                 afsk_live_tx_submit_events_rated (rate="heard") of the same list
The uniform-group and the mixed-group pulls are checked to write identical samples before anything is timed.
--json / --txt append this run to OUT when it exists."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from afskmodem_amd import _native, live  # noqa: E402
from afskmodem_amd.live import LiveTransmitter  # noqa: E402

STEPS = {"pull2048": 300, "pull8192": 300, "submit": 180, "relay": 180}     # step -> its time limit in seconds
BAUDS = (300, 1200, 2400)
DEPTH, PAYLOAD, TRAINING = 4, 24, 0.5
# the shortest queue: four 2400-baud messages of 20 * (1200 + 4 + 14 * 24) + 4800 samples
SHORTEST = DEPTH * (20 * (1200 + 4 + 14 * PAYLOAD) + 4800)


class Library:
    """One build of the library, bound like _native.lib(); entries a build lacks (the parent's) stay unbound."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        for table in (getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES")):
            for name, (res, args) in table.items():
                if hasattr(self.L, name):
                    fn = getattr(self.L, name)
                    fn.restype, fn.argtypes = res, args

    def __getattr__(self, name):
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


def stats(us):
    us = np.asarray(us)
    return dict(us_mean=round(float(us.mean()), 2), us_median=round(float(np.median(us)), 2),
                us_p90=round(float(np.percentile(us, 90)), 2), samples=int(us.size))


def timed(torch, graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    return a, b


def capture(torch, fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn(side)
    torch.cuda.synchronize()
    return g


class Messages:
    """`per_channel` messages of PAYLOAD bytes on every channel as the device arrays of a submit, sorted by channel."""

    def __init__(self, torch, n, per_channel, seed=7):
        rng = np.random.default_rng(seed)
        m = n * per_channel
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.m = m
        self.channel = dev(np.repeat(np.arange(n, dtype=np.int32), per_channel))
        self.offset = dev(np.arange(m, dtype=np.int64) * PAYLOAD)
        self.length = dev(np.full(m, PAYLOAD, np.int32))
        self.payload = dev(rng.integers(0, 256, m * PAYLOAD, dtype=np.uint8))
        c, k = np.repeat(np.arange(n), per_channel), np.tile(np.arange(per_channel), n)
        self.rate = {"zero": dev(np.zeros(m, np.int32)), "fixed": dev((c % 3).astype(np.int32)),
                     "rotating": dev(((c + k) % 3).astype(np.int32))}
        self.out = (torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int64, device="cuda"),
                    torch.zeros(m, dtype=torch.int32, device="cuda"))

    def submit(self, lib, tx, rate=None, stream=None):
        s = None if stream is None else C.c_void_p(stream.cuda_stream)
        outs = [t.data_ptr() for t in self.out]
        if rate is None:
            rc = lib.afsk_live_tx_submit(tx.handle, self.m, self.channel.data_ptr(), self.offset.data_ptr(),
                                         self.length.data_ptr(), self.payload.data_ptr(), None, *outs, s)
        else:
            rc = lib.afsk_live_tx_submit_rated(tx.handle, self.m, self.channel.data_ptr(), self.rate[rate].data_ptr(),
                                               self.offset.data_ptr(), self.length.data_ptr(), self.payload.data_ptr(),
                                               None, *outs, s)
        _native.check(rc)


def make_tx(lib, kind, n):
    kw = dict(queue_depth=DEPTH, max_payload_len=PAYLOAD)
    with using(lib):
        if kind == "uniform":
            return LiveTransmitter(n, 1200, TRAINING, **kw)
        if kind == "mixed":
            return LiveTransmitter(n, [BAUDS[c % 3] for c in range(n)], TRAINING, **kw)
        if kind == "rated1":
            return LiveTransmitter(n, rates=[1200], training_time=TRAINING, **kw)
        return LiveTransmitter(n, rates=list(BAUDS), training_time=TRAINING, **kw)


def close_all(torch, variants):
    """Every variant's graph dropped and its transmitter destroyed by the library that created it."""
    torch.cuda.synchronize()
    while variants:
        name, lib, tx, _, g = variants.pop()
        del g
        with using(lib):
            tx.close()


def rotate(torch, variants, reps, one_pass):
    """reps + 1 passes (the first is a warm-up), every pass one variant later; one_pass(variant) -> [(start, end)]."""
    us = {name: [] for name, *_ in variants}
    for r in range(reps + 1):
        for i in range(len(variants)):
            v = variants[(i + r) % len(variants)]
            events = one_pass(v)
            torch.cuda.synchronize()
            if r > 0:
                us[v[0]] += [a.elapsed_time(b) * 1e3 for a, b in events]
    return us


def report(step, shape, us, pairs, lines, results):
    """The records of one step, and for every (variant, baseline) of `pairs` the ratio of the means next to the spread
    of the two parent copies, when there are any."""
    recs = {name: dict(step=step, shape=shape, variant=name, **stats(v)) for name, v in us.items()}
    for r in recs.values():
        print(json.dumps(r), flush=True)
        results.append(r)
    spread = None
    if "parent" in recs and "parent2" in recs:
        spread = abs(recs["parent2"]["us_mean"] / recs["parent"]["us_mean"] - 1.0)
        lines.append(f"{step:9s} {shape:12s} parent {recs['parent']['us_mean']:8.1f} / {recs['parent']['us_median']:8.1f} us "
                     f"(mean / median)   parent2 {recs['parent2']['us_mean']:8.1f} / {recs['parent2']['us_median']:8.1f}"
                     f"   spread {100 * spread:.2f} %")
    for name, base in pairs:
        if name not in recs or base not in recs:
            continue
        ratio = recs[name]["us_mean"] / recs[base]["us_mean"]
        cmp_ = dict(step=step, shape=shape, variant=name, baseline=base, over_baseline_mean=round(ratio, 4),
                    over_baseline_median=round(recs[name]["us_median"] / recs[base]["us_median"], 4))
        verdict = ""
        if spread is not None:
            cmp_.update(parent_spread=round(spread, 4), inside_spread=bool(abs(ratio - 1.0) <= spread))
            verdict = "   inside the parent's spread" if cmp_["inside_spread"] else "   OUTSIDE the parent's spread"
        print(json.dumps(cmp_), flush=True)
        results.append(cmp_)
        lines.append(f"{'':9s} {'':12s} {name:16s} {recs[name]['us_mean']:8.1f} / {recs[name]['us_median']:8.1f} us   "
                     f"x{ratio:.3f} of {base} (median x{cmp_['over_baseline_median']:.3f}){verdict}")


def step_pull(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = Messages(torch, n, DEPTH)
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    pulls = min(SHORTEST // T, 48)                     # timed pulls per pass: inside the shortest queue
    plan = [("uniform", this, "uniform", None), ("mixed", this, "mixed", None), ("rated1", this, "rated1", "zero"),
            ("rated3_fixed", this, "rated3", "fixed"), ("rated3_rotating", this, "rated3", "rotating")]
    if "parent" in libs:
        plan = [("parent", libs["parent"], "uniform", None), ("parent_mixed", libs["parent"], "mixed", None)] + plan \
            + [("parent2", libs["parent2"], "uniform", None), ("parent_mixed2", libs["parent2"], "mixed", None)]
    variants = []
    for name, lib, kind, rate in plan:
        tx = make_tx(lib, kind, n)
        with using(lib):
            g = capture(torch, lambda side: tx.pull(T, out=buf, stream=side))
        variants.append((name, lib, tx, rate, g))

    def refill(v):
        name, lib, tx, rate, g = v
        with using(lib):
            tx.reset()
        msgs.submit(lib, tx, rate)

    # the same samples within a group, before anything is timed: three pulls into the shared buffer
    for group in (("parent", "parent2", "uniform", "rated1"), ("parent_mixed", "parent_mixed2", "mixed", "rated3_fixed")):
        ref = None
        for v in variants:
            if v[0] in group:
                refill(v)
                for _ in range(3):
                    v[4].replay()
                torch.cuda.synchronize()
                assert int(msgs.out[0].abs().sum()) == 0, (v[0], "a message was refused")
                if ref is None:
                    ref = buf.clone()
                    assert bool(ref.any())
                else:
                    assert torch.equal(buf, ref), (v[0], "renders other samples than its group")
        del ref

    def one_pass(v):
        refill(v)
        return [timed(torch, v[4]) for _ in range(pulls)]

    us = rotate(torch, variants, reps, one_pass)
    report(f"pull{T}", f"{n}x{T}", us, [("parent2", "parent"), ("uniform", "parent"), ("rated1", "uniform")],
           lines, results)
    # the mixed pulls against the spread of the parent's own two MIXED copies
    mixed = {k.replace("parent_mixed", "parent"): v for k, v in us.items() if k not in ("parent", "parent2")}
    report(f"pull{T}", f"{n}x{T} mixed", mixed, [("parent2", "parent"), ("mixed", "parent"), ("rated3_fixed", "mixed"),
                                                 ("rated3_rotating", "mixed"), ("rated3_rotating", "rated3_fixed")],
           lines, results)
    close_all(torch, variants)


def step_submit(torch, libs, n, reps, lines, results):
    this = libs["this"]
    msgs = Messages(torch, n, 1)
    plan = [("submit", this, "uniform", None), ("submit_rated", this, "rated1", "zero")]
    if "parent" in libs:
        plan = [("parent", libs["parent"], "uniform", None)] + plan + [("parent2", libs["parent2"], "uniform", None)]
    variants = []
    for name, lib, kind, rate in plan:
        tx = make_tx(lib, kind, n)
        g = capture(torch, lambda side: msgs.submit(lib, tx, rate, side))
        variants.append((name, lib, tx, rate, g))

    def one_pass(v):
        events = []
        for _ in range(8):
            with using(v[1]):
                v[2].reset()                           # (untimed: the queues take the messages again)
            events.append(timed(torch, v[4]))
        torch.cuda.synchronize()
        assert int(msgs.out[0].abs().sum()) == 0, (v[0], "a message was refused")
        return events

    us = rotate(torch, variants, reps, one_pass)
    report("submit", f"{n} msgs", us, [("parent2", "parent"), ("submit", "parent"), ("submit_rated", "submit")],
           lines, results)
    close_all(torch, variants)


def packed_events(torch, n, closed, slots=2, nbytes=16, seed=11):
    """An events buffer as afsk_live_pack leaves it: channels 0, n / closed, ... closed one burst of `nbytes` bytes
    each (slot 0, status OK); and the rates an auto receiver's push would have left, int32 [n, slots]."""
    max_events, max_bytes = n * slots, n * slots * nbytes
    ro, po, total = live.events_layout(n, slots, max_events, max_bytes)
    host = np.zeros(total, np.uint8)
    header = np.zeros(1, live.EVENTS_HEADER_DTYPE)
    header["count"], header["stored"], header["n_bytes"], header["stored_bytes"] = closed, closed, closed * nbytes, \
        closed * nbytes
    host[: header.nbytes] = header.view(np.uint8)
    recs = np.zeros(closed, live.EVENT_DTYPE)
    recs["channel"] = np.arange(closed) * (n // closed)
    recs["burst_len"], recs["nbytes"], recs["nbits"] = 2048, nbytes, 8 * nbytes
    recs["payload_offset"] = np.arange(closed) * nbytes
    host[ro: ro + recs.nbytes] = recs.view(np.uint8)
    host[po: po + closed * nbytes] = np.random.default_rng(seed).integers(0, 256, closed * nbytes, dtype=np.uint8)
    rx_bf = np.zeros((n, slots), np.int32)
    rx_bf[:, 0] = np.asarray([160, 40, 20], np.int32)[np.arange(n) % 3]
    return torch.from_numpy(host).cuda(), max_events, max_bytes, nbytes, torch.from_numpy(rx_bf).cuda()


def step_relay(torch, libs, n, reps, lines, results):
    this = libs["this"]
    for closed in (64, n):
        buf, me, mb, stride, rx_bf = packed_events(torch, n, closed)
        outs = (torch.zeros(me, dtype=torch.int32, device="cuda"), torch.zeros(me, dtype=torch.int64, device="cuda"),
                torch.zeros(me, dtype=torch.int32, device="cuda"))
        optr = [t.data_ptr() for t in outs]
        plan = [("events", this, "uniform", False), ("events_heard", this, "rated3", True)]
        if "parent" in libs:
            plan = [("parent", libs["parent"], "uniform", False)] + plan \
                + [("parent2", libs["parent2"], "uniform", False)]
        variants = []
        for name, lib, kind, heard in plan:
            tx = make_tx(lib, kind, n)

            def call(side, lib=lib, tx=tx, heard=heard):
                s = C.c_void_p(side.cuda_stream)
                if heard:
                    rc = lib.afsk_live_tx_submit_events_rated(tx.handle, buf.data_ptr(), me, mb, stride, n, None, 1,
                                                              rx_bf.data_ptr(), 2, *optr, s)
                else:
                    rc = lib.afsk_live_tx_submit_events(tx.handle, buf.data_ptr(), me, mb, stride, n, None, 1, *optr, s)
                _native.check(rc)
            variants.append((name, lib, tx, heard, capture(torch, call)))

        def one_pass(v):
            events = []
            for _ in range(8):
                with using(v[1]):
                    v[2].reset()
                events.append(timed(torch, v[4]))
            torch.cuda.synchronize()
            st = outs[0]
            assert int((st == _native.LIVE_TX_QUEUED).sum()) == closed and int((st == _native.LIVE_TX_NONE).sum()) == \
                me - closed, (v[0], "not every closed burst was queued")
            return events

        us = rotate(torch, variants, reps, one_pass)
        report("relay", f"{closed} of {n}", us, [("parent2", "parent"), ("events", "parent"),
                                                 ("events_heard", "events")], lines, results)
        close_all(torch, variants)


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": Library(_native.LIB_PATH)}
    tmp = None
    if args.parent:
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = Library(args.parent), Library(twin)
    lines, results = [], []
    if args.step.startswith("pull"):
        step_pull(torch, libs, args.channels, int(args.step[4:]), args.reps, lines, results)
    elif args.step == "submit":
        step_submit(torch, libs, args.channels, args.reps, lines, results)
    else:
        step_relay(torch, libs, args.channels, args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_tx_rated_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(step=args.step, channels=args.channels, reps=args.reps, parent=bool(args.parent),
                                results=results))
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (AFSK_AMD_LIB names another build as this one)")
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    # the driver: every step a fresh process under its own time limit, the chain ends at the first failure
    for step in ("pull2048", "pull8192", "submit", "relay"):
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
