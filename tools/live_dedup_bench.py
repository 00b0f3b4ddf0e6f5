#!/usr/bin/env python3
"""live_dedup_bench.py -- what the duplicate filter (afsk_live_dedup_filter, live.LiveDedup) costs next to the relay that
reads the same list, what submit_events(keep=) costs next to submit_events, what the filter adds to a station's one-graph
tick, and what the one added include line did to the pull, the relay and the push.

    python tools/live_dedup_bench.py [--parent PARENT.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_dedup_bench.py --step filter24|filter256|tick2048|tick8192|pull2048|pull8192|push2048 ...

Without --step the tool is a driver shaped like tools/live_mix_bench.py (whose helpers' homes, tools/live_csma_bench.py
and tools/live_tx_rated_bench.py, it uses): the steps run one after the other, each as a fresh child process under its
own `timeout`, and the chain stops at the first one that fails -- nothing more is started on the GPU after a fault, an
abort or a time limit.  A step compares all its variants in ONE process over the same buffers: every variant's call is
captured once into a HIP graph and replayed, HIP events around each replay give the time, and the passes take turns.

Steps (n = --channels receiver channels):
  filter24 / filter256   an events buffer as a pack leaves it with 64 and with n closed bursts of 24 / 256 bytes (slot 0
          of every n / closed-th channel), depth 8:
            events       afsk_live_tx_submit_events on a uniform 1200-baud transmitter, reset before every replay
            kept         afsk_live_tx_submit_events_kept with a keep array of all ones, likewise
            filter       afsk_live_dedup_filter on rings emptied before every replay: every burst is NEW and inserted
            filter_dup   the same without the reset: every burst is a DUP, nothing is stored
            parent / parent2   `events` from --parent, loaded twice: the spread identical code shows in this run
  tick    one graph per tick, wall clock until the device is done: push(events=, mute=on_air) -> busy [-> filter] ->
          submit_events([keep=]) -> pull(out=src rows, hold=busy, persist=63, slot=4800) -> medium.mix (the station and a
          carrier on every 64th row), T = 2048 or 8192
            plain / dedup   without and with the filter
  pull, push   tools/live_csma_bench.py's steps of the same name against --parent: the kernels next to the new include line
--json / --txt append this run to OUT when it exists."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import live_csma_bench as CB  # noqa: E402
import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native  # noqa: E402
from afskmodem_amd.live import LiveDedup, LiveMedium, LiveReceiver, LiveTransmitter  # noqa: E402

STEPS = {"filter24": 300, "filter256": 300, "tick2048": 300, "tick8192": 300, "pull2048": 300, "pull8192": 300,
         "push2048": 300}
DEPTH = 8


def step_filter(torch, libs, n, nbytes, reps, lines, results):
    this = libs["this"]
    for closed in (64, n):
        buf, me, mb, stride, _ = B.packed_events(torch, n, closed, nbytes=nbytes)
        outs = (torch.zeros(me, dtype=torch.int32, device="cuda"), torch.zeros(me, dtype=torch.int64, device="cuda"),
                torch.zeros(me, dtype=torch.int32, device="cuda"))
        optr = [t.data_ptr() for t in outs]
        keep = torch.ones(me, dtype=torch.int32, device="cuda")
        verdict = torch.zeros(me, dtype=torch.int32, device="cuda")
        plan = [("events", this), ("kept", this)]
        if "parent" in libs:
            plan = [("parent", libs["parent"])] + plan + [("parent2", libs["parent2"])]
        variants = []
        for name, lib in plan:
            with B.using(lib):
                tx = LiveTransmitter(n, 1200, B.TRAINING, queue_depth=B.DEPTH, max_payload_len=nbytes)

            def call(side, lib=lib, tx=tx, kept=name == "kept"):
                s = C.c_void_p(side.cuda_stream)
                if kept:
                    rc = lib.afsk_live_tx_submit_events_kept(tx.handle, buf.data_ptr(), me, mb, stride, n, None, 1, None,
                                                             0, keep.data_ptr(), *optr, s)
                else:
                    rc = lib.afsk_live_tx_submit_events(tx.handle, buf.data_ptr(), me, mb, stride, n, None, 1, *optr, s)
                _native.check(rc)
            variants.append((name, lib, tx, "relay", B.capture(torch, call)))
        for name in ("filter", "filter_dup"):
            dd = LiveDedup(n, depth=DEPTH, window=30.0)

            def call(side, dd=dd):
                _native.check(this.afsk_live_dedup_filter(dd.handle, buf.data_ptr(), me, mb, stride, 1, dd.window,
                                                          verdict.data_ptr(), C.c_void_p(side.cuda_stream)))
            variants.append((name, this, dd, name, B.capture(torch, call)))

        def one_pass(v):
            events = []
            for _ in range(8):
                if v[3] != "filter_dup":
                    with B.using(v[1]):
                        v[2].reset()
                events.append(B.timed(torch, v[4]))
            torch.cuda.synchronize()
            if v[3] == "relay":
                st = outs[0]
                assert int((st == _native.LIVE_TX_QUEUED).sum()) == closed and \
                    int((st == _native.LIVE_TX_NONE).sum()) == me - closed, (v[0], "not every closed burst was queued")
            else:
                want = _native.LIVE_DEDUP_NEW if v[3] == "filter" else _native.LIVE_DEDUP_DUP
                assert int((verdict == want).sum()) == closed and \
                    int((verdict == _native.LIVE_DEDUP_NONE).sum()) == me - closed, (v[0], "unexpected verdicts")
            return events

        with B.using(this):                                      # filter_dup: the rings hold every burst from here on
            variants[-1][4].replay()
        torch.cuda.synchronize()
        us = B.rotate(torch, variants, reps, one_pass)
        B.report(f"filter{nbytes}", f"{closed} of {n}", us,
                 [("parent2", "parent"), ("events", "parent"), ("kept", "events"), ("filter", "events"),
                  ("filter_dup", "events")], lines, results)
        B.close_all(torch, variants)


def step_tick(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, CB.DEPTH)
    carrier = CB.carrier(torch, n, T)
    ticks = min(CB.DEPTH * CB.MESSAGE // T, 32)
    variants = {}
    for name in ("plain", "dedup"):
        rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=32)
        tx = CB.make_tx(this, n)
        res, ev = rx.alloc_result(), rx.alloc_events(max_events=4096, max_bytes=4096 * 32)
        sub = tx.alloc_submit_result(ev.max_events)
        dd = rx.deduper(depth=DEPTH, window=30.0) if name == "dedup" else None
        keep = dd.alloc_verdict(ev.max_events) if dd is not None else None
        busy = torch.zeros(n, dtype=torch.int32, device="cuda")
        src = torch.zeros((2 * n, T), dtype=torch.int16, device="cuda")         # the station's rows | the carrier's
        src[n:].copy_(carrier)
        chunk = torch.zeros((n, T), dtype=torch.int16, device="cuda")
        medium = LiveMedium.from_matrix([[1.0]], n, extra=1)

        def tick(side, rx=rx, tx=tx, res=res, ev=ev, sub=sub, busy=busy, src=src, chunk=chunk, medium=medium, dd=dd,
                 keep=keep):
            rx.push(chunk, out=res, events=ev, mute=tx.on_air, stream=side)
            rx.busy(out=busy, stream=side)
            if dd is not None:
                dd.filter(ev, out=keep, stream=side)
            tx.submit_events(ev, out=sub, keep=keep, stream=side)
            tx.pull(T, out=src[:n], hold=busy, holdoff=4800, persist=63, stream=side, **CB.CSMA)
            medium.mix(src, out=chunk, stream=side)

        # (everything the graph's launches read or write stays referenced for as long as the graph does)
        variants[name] = (rx, tx, dd, busy, src, chunk, (medium, res, ev, sub, keep), B.capture(torch, tick))

    def one_pass(name):
        rx, tx, dd, busy, src, chunk, _, graph = variants[name]
        rx.reset()
        tx.reset()
        tx.on_air.zero_()
        if dd is not None:
            dd.reset()
        src[:n].zero_()
        chunk.zero_()
        msgs.submit(this, tx, None)
        torch.cuda.synchronize()
        us = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        assert int(busy.sum()) >= n // 64, (name, "every 64th channel hears the carrier")
        return us, chunk.clone()

    us = {name: [] for name in variants}
    order, last = list(variants), {}
    for r in range(reps + 1):
        for i in range(len(order)):
            name = order[(i + r) % len(order)]
            got, last[name] = one_pass(name)
            if r > 0:
                us[name] += got
    assert torch.equal(last["plain"], last["dedup"]), "the two ticks left different media"
    base = B.stats(us["plain"])
    lines.append(f"{'tick' + str(T):9s} {n}x{T}   plain {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"wall clock until the device is done, {base['samples']} ticks)")
    B.report(f"tick{T}", f"{n}x{T} wall", us, [("dedup", "plain")], lines, results)
    torch.cuda.synchronize()
    for rx, tx, dd, *_, graph in variants.values():
        del graph
        rx.close()
        tx.close()
        if dd is not None:
            dd.close()


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": B.Library(_native.LIB_PATH)}
    name = args.step.rstrip("0123456789")
    size = int(args.step[len(name):])
    tmp = None
    if args.parent and name in ("pull", "push", "filter"):
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = B.Library(args.parent), B.Library(twin)
    lines, results = [], []
    if name == "filter":
        step_filter(torch, libs, args.channels, size, args.reps, lines, results)
    elif name == "tick":
        step_tick(torch, libs, args.channels, size, args.reps, lines, results)
    elif name == "pull":
        CB.step_pull(torch, libs, args.channels, size, args.reps, lines, results)
    else:
        CB.step_push(torch, libs, "stream", args.channels, size, args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_dedup_bench.py", runs=[])
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (the relay, the pull and the push are compared against it)")
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
        if step.rstrip("0123456789") in ("pull", "push") and not args.parent:
            continue
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
