#!/usr/bin/env python3
"""live_hold_bench.py -- what carrier sense costs the live side (afsk_live_busy, afsk_live_tx_pull_hold), step by step.

    python tools/live_hold_bench.py [--parent PARENT.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_hold_bench.py --step pull2048|pull8192|busy|tick2048|tick8192 ...    (one step, in this process)

Without --step the tool is a driver, shaped like tools/live_tx_rated_bench.py (whose helpers it uses): it runs the steps
one after the other, each as a fresh child process under its own `timeout`, and stops at the first one that fails --
nothing more is started on the GPU after a fault, an abort or a time limit.  A step compares all its variants in ONE
process over the same buffers: every variant's call is captured once into a HIP graph and replayed, HIP events around
each replay give the time, and the passes take turns (every pass starts one variant later).

The workload is tools/live_bench.py's: 1200 baud, training 0.5 s, payloads of 24 bytes, every channel busy.  Before
each pass a variant's queues are refilled (reset + a submit of queue_depth messages per channel, untimed).

Variants (--parent names a libafsk_amd.so of the parent commit, loaded twice -- the second time as a copy under
another name -- and the difference of the two copies is the spread identical code shows in this run):
  pull     parent / parent2 / plain    LiveTransmitter(n, 1200).pull(T)           of the parent (twice) and of this build
           hold_none                   pull(T, hold=h) with h all 0                against plain
           hold_1in64                  ... with every 64th channel held
           hold_all                    ... with every channel held (nothing starts: the rows are zeros)
           The plain, parent and hold_none pulls are checked to write identical samples before anything is timed.
  busy     busy                        LiveReceiver(n, 1200, streaming).busy(out=) alone
  tick     one_graph                   push(events=) -> busy(out=) -> submit_events(out=) -> pull(out=, hold=busy) as
                                       ONE graph replay per tick (every 64th channel hears a carrier and is held)
           host_read                   the same tick with busy copied to the host in the middle: graph(push, busy),
                                       busy.cpu(), graph(submit_events, pull(hold=busy)) -- wall clock, as one_graph
--json / --txt append this run to OUT when it exists."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native  # noqa: E402
from afskmodem_amd.live import LiveReceiver, LiveTransmitter  # noqa: E402

STEPS = {"pull2048": 300, "pull8192": 300, "busy": 120, "tick2048": 240, "tick8192": 300}   # step -> seconds allowed
DEPTH, PAYLOAD, TRAINING = B.DEPTH, B.PAYLOAD, B.TRAINING
MESSAGE = 40 * (600 + 4 + 14 * PAYLOAD) + 4800               # samples of one 1200-baud message


def make_tx(lib, n):
    with B.using(lib):
        return LiveTransmitter(n, 1200, TRAINING, queue_depth=DEPTH, max_payload_len=PAYLOAD)


def step_pull(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, DEPTH)
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    pulls = min(DEPTH * MESSAGE // T, 48)                     # timed pulls per pass: inside the queue
    holds = {"hold_none": torch.zeros(n, dtype=torch.int32, device="cuda"),
             "hold_1in64": (torch.arange(n, device="cuda") % 64 == 0).to(torch.int32),
             "hold_all": torch.ones(n, dtype=torch.int32, device="cuda")}
    plan = [("plain", this, None)] + [(name, this, h) for name, h in holds.items()]
    if "parent" in libs:
        plan = [("parent", libs["parent"], None)] + plan + [("parent2", libs["parent2"], None)]
    variants = []
    for name, lib, hold in plan:
        tx = make_tx(lib, n)
        with B.using(lib):
            g = B.capture(torch, lambda side: tx.pull(T, out=buf, stream=side) if hold is None
                          else tx.pull(T, out=buf, stream=side, hold=hold, holdoff=0))
        variants.append((name, lib, tx, None, g))

    def refill(v):
        with B.using(v[1]):
            v[2].reset()
        msgs.submit(v[1], v[2], None)

    ref = None                                                # the same samples, before anything is timed
    for v in variants:
        if v[0] in ("parent", "parent2", "plain", "hold_none"):
            refill(v)
            for _ in range(3):
                v[4].replay()
            torch.cuda.synchronize()
            assert int(msgs.out[0].abs().sum()) == 0, (v[0], "a message was refused")
            if ref is None:
                ref = buf.clone()
                assert bool(ref.any())
            else:
                assert torch.equal(buf, ref), (v[0], "renders other samples than the plain pull")
    del ref

    def one_pass(v):
        refill(v)
        return [B.timed(torch, v[4]) for _ in range(pulls)]

    us = B.rotate(torch, variants, reps, one_pass)
    B.report(f"pull{T}", f"{n}x{T}", us, [("parent2", "parent"), ("plain", "parent"), ("hold_none", "plain"),
                                          ("hold_1in64", "plain"), ("hold_all", "plain")], lines, results)
    B.close_all(torch, variants)


def carrier(torch, n, T):
    """[n, T] int16: every 64th channel hears a full-scale square wave (its gate opens and stays open), the rest silence."""
    chunk = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    wave = torch.tensor([20000, -20000], dtype=torch.int16, device="cuda").repeat(T // 2)
    chunk[::64] = wave
    return chunk


def step_busy(torch, libs, n, reps, lines, results):
    rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=2048, max_payload_len=32)
    rx.push(carrier(torch, n, 2048))
    rx.push(carrier(torch, n, 2048))
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    g = B.capture(torch, lambda side: rx.busy(out=out, stream=side))
    g.replay()
    torch.cuda.synchronize()
    assert int(out.sum()) == n // 64, "every 64th channel is recording"
    us = []
    for r in range(reps + 1):
        events = [B.timed(torch, g) for _ in range(48)]
        torch.cuda.synchronize()
        if r > 0:
            us += [a.elapsed_time(b) * 1e3 for a, b in events]
    B.report("busy", f"{n} channels", {"busy": us}, [], lines, results)
    lines.append(f"{'busy':9s} {n} channels   {B.stats(us)['us_mean']:8.1f} / {B.stats(us)['us_median']:8.1f} us "
                 f"(mean / median) per graph replay of afsk_live_busy")
    torch.cuda.synchronize()
    del g
    rx.close()


def step_tick(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, DEPTH)
    chunk = carrier(torch, n, T)
    pulled = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    ticks = min(DEPTH * MESSAGE // T, 32)
    variants = {}
    for name in ("one_graph", "host_read"):
        rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=32)
        tx = make_tx(this, n)
        res, ev = rx.alloc_result(), rx.alloc_events(max_events=4096, max_bytes=4096 * 32)
        sub = tx.alloc_submit_result(ev.max_events)
        busy = torch.zeros(n, dtype=torch.int32, device="cuda")

        def front(side, rx=rx, res=res, ev=ev, busy=busy):
            rx.push(chunk, out=res, events=ev, stream=side)
            rx.busy(out=busy, stream=side)

        def back(side, tx=tx, ev=ev, sub=sub, busy=busy):
            tx.submit_events(ev, out=sub, stream=side)
            tx.pull(T, out=pulled, hold=busy, holdoff=4800, stream=side)

        if name == "one_graph":
            graphs = (B.capture(torch, lambda side: (front(side), back(side))),)
        else:
            graphs = (B.capture(torch, front), B.capture(torch, back))
        variants[name] = (rx, tx, busy, graphs)

    def one_pass(name):
        rx, tx, busy, graphs = variants[name]
        rx.reset()
        tx.reset()
        msgs.submit(this, tx, None)
        torch.cuda.synchronize()
        us = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            graphs[0].replay()
            if len(graphs) == 2:
                host = busy.cpu()                             # the host hop this feature removes
                graphs[1].replay()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        assert int(busy.sum()) == n // 64, (name, "every 64th channel is held")
        if len(graphs) == 2:
            assert int(host.sum()) == n // 64
        return us

    us = {name: [] for name in variants}
    order = list(variants)
    for r in range(reps + 1):
        for i in range(len(order)):
            name = order[(i + r) % len(order)]
            got = one_pass(name)
            if r > 0:
                us[name] += got
    one = B.stats(us["one_graph"])
    lines.append(f"{'tick' + str(T):9s} {n}x{T}   one_graph {one['us_mean']:8.1f} / {one['us_median']:8.1f} us (mean / median, "
                 f"wall clock until the device is done, {one['samples']} ticks)")
    B.report(f"tick{T}", f"{n}x{T} wall", us, [("host_read", "one_graph")], lines, results)
    torch.cuda.synchronize()
    for rx, tx, _, graphs in variants.values():
        del graphs
        rx.close()
        tx.close()


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": B.Library(_native.LIB_PATH)}
    tmp = None
    if args.parent and args.step.startswith("pull"):
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = B.Library(args.parent), B.Library(twin)
    lines, results = [], []
    if args.step.startswith("pull"):
        step_pull(torch, libs, args.channels, int(args.step[4:]), args.reps, lines, results)
    elif args.step == "busy":
        step_busy(torch, libs, args.channels, args.reps, lines, results)
    else:
        step_tick(torch, libs, args.channels, int(args.step[4:]), args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_hold_bench.py", runs=[])
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (the pull steps compare against it)")
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    # the driver: every step a fresh process under its own time limit, the chain ends at the first failure
    for step in STEPS:
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
