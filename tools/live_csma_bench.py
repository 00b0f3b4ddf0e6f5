#!/usr/bin/env python3
"""live_csma_bench.py -- what the half-duplex additions cost the live side (afsk_live_tx_pull_csma, afsk_live_push_muted,
afsk_live_push_auto_muted), step by step.

    python tools/live_csma_bench.py [--parent PARENT.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_csma_bench.py --step pull2048|pull8192|push2048|...|tick8192 ...    (one step, in this process)

Without --step the tool is a driver, shaped like tools/live_hold_bench.py (whose helpers in tools/live_tx_rated_bench.py
it uses): it runs the steps one after the other, each as a fresh child process under its own `timeout`, and stops at the
first one that fails -- nothing more is started on the GPU after a fault, an abort or a time limit.  A step compares all
its variants in ONE process over the same buffers: every variant's call is captured once into a HIP graph and replayed,
HIP events around each replay give the time, and the passes take turns (every pass starts one variant later).

The workload is tools/live_bench.py's: 1200 baud, training 0.5 s, payloads of 24 bytes, every channel busy.  Before each
pass a transmitter's queues are refilled (reset + a submit of queue_depth messages per channel, untimed) and a receiver is
reset; a receiver is then pushed the first T samples of such a message over and over.

Variants (--parent names a libafsk_amd.so of the parent commit, loaded twice -- the second time as a copy under another
name -- and the difference of the two copies is the spread identical code shows in this run):
  pull        parent / parent2 / plain       pull(T) of the parent (twice) and of this build
              parent_hold / hold_none        pull(T, hold=h), h all 0, of the parent and of this build
              hold_1in64 / hold_all          ... every 64th channel / every channel held
              csma255_* / csma0_*            pull(T, hold=h, persist=255 | 0, slot=4800, seed=1) with the same three h;
                                             persist 0 with all held is the worst case, 255 draws per channel
  push        parent / parent2 / ragged      push(chunk, lengths=) of a streaming receiver, parent (twice) and this build
              mute_none / _1in64 / _all      push(chunk, lengths=, mute=m): m all (0, 0); (0, T) on every 64th; (0, T)
  pushstored  parent / parent2 / ragged      the same six of a stored receiver (its demodulator launch included)
              mute_none / _1in64 / _all
  pushauto    ragged / mute_*                the auto-rate receiver with four candidates: afsk_live_push_auto against
                                             afsk_live_push_auto_muted
  tick        hold / csma                    push(events=) -> busy -> submit_events -> pull(hold=busy) against
                                             push(events=, mute=tx.on_air) -> ... -> pull(hold=busy, persist=63, slot=4800,
                                             seed=1), each ONE graph replay per tick, wall clock until the device is done
--json / --txt append this run to OUT when it exists."""
import argparse
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

import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native  # noqa: E402
from afskmodem_amd.live import LiveReceiver, LiveTransmitter  # noqa: E402

SIZES = (2048, 8192)
STEPS = {f"{s}{T}": 300 for s in ("pull", "push", "pushstored", "pushauto", "tick") for T in SIZES}
DEPTH, PAYLOAD, TRAINING = B.DEPTH, B.PAYLOAD, B.TRAINING
MESSAGE = 40 * (600 + 4 + 14 * PAYLOAD) + 4800               # samples of one 1200-baud message
CSMA = dict(slot=4800, seed=1)


def make_tx(lib, n):
    with B.using(lib):
        return LiveTransmitter(n, 1200, TRAINING, queue_depth=DEPTH, max_payload_len=PAYLOAD)


def every(torch, n, k):
    return (torch.arange(n, device="cuda") % k == 0).to(torch.int32)


def step_pull(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, DEPTH)
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    pulls = min(DEPTH * MESSAGE // T, 48)                     # timed pulls per pass: inside the queue
    holds = {"none": torch.zeros(n, dtype=torch.int32, device="cuda"), "1in64": every(torch, n, 64),
             "all": torch.ones(n, dtype=torch.int32, device="cuda")}
    plan = [("plain", this, None, None)]
    plan += [(f"hold_{k}", this, h, None) for k, h in holds.items()]
    plan += [(f"csma{p}_{k}", this, h, p) for p in (255, 0) for k, h in holds.items()]
    if "parent" in libs:
        plan = [("parent", libs["parent"], None, None), ("parent_hold", libs["parent"], holds["none"], None)] + plan \
            + [("parent2", libs["parent2"], None, None)]
    variants = []
    for name, lib, hold, persist in plan:
        tx = make_tx(lib, n)

        def call(side, tx=tx, hold=hold, persist=persist):
            if hold is None:
                tx.pull(T, out=buf, stream=side)
            elif persist is None:
                tx.pull(T, out=buf, stream=side, hold=hold, holdoff=0)
            else:
                tx.pull(T, out=buf, stream=side, hold=hold, holdoff=0, persist=persist, **CSMA)

        with B.using(lib):
            g = B.capture(torch, call)
        variants.append((name, lib, tx, None, g))

    def refill(v):
        with B.using(v[1]):
            v[2].reset()
        msgs.submit(v[1], v[2], None)

    ref = None                                                # the same samples, before anything is timed
    for v in variants:
        if v[0] in ("parent", "parent2", "parent_hold", "plain", "hold_none", "csma255_none", "csma0_none"):
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
    pairs = [("parent2", "parent"), ("plain", "parent"), ("hold_none", "parent_hold")]
    pairs += [(f"csma{p}_{k}", f"hold_{k}") for p in (255, 0) for k in holds]
    B.report(f"pull{T}", f"{n}x{T}", us, pairs, lines, results)
    B.close_all(torch, variants)


def message_chunk(torch, this, n, T):
    """[n, T] int16: the first T samples of a 1200-baud message on every channel (rendered by this build's plain pull)."""
    msgs = B.Messages(torch, n, 1)
    tx = make_tx(this, n)
    msgs.submit(this, tx, None)
    chunk = tx.pull(T).clone()
    torch.cuda.synchronize()
    tx.close()
    assert bool(chunk.any())
    return chunk


def make_rx(lib, kind, n, T):
    with B.using(lib):
        if kind == "stored":
            return LiveReceiver(n, 40, max_burst_len=65536, max_chunk_len=T)
        if kind == "auto":
            return LiveReceiver(n, "auto", max_burst_len=None, max_chunk_len=T, max_payload_len=32,
                                candidates=[160, 40, 20, 8])
        return LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=32)


def step_push(torch, libs, kind, n, T, reps, lines, results):
    this = libs["this"]
    chunk = message_chunk(torch, this, n, T)
    lens = torch.full((n,), T, dtype=torch.int32, device="cuda")
    pushes = 32
    full = torch.tensor([0, T], dtype=torch.int32, device="cuda")
    mutes = {"mute_none": torch.zeros((n, 2), dtype=torch.int32, device="cuda"),
             "mute_1in64": (every(torch, n, 64)[:, None] * full[None, :]).contiguous(),
             "mute_all": full[None, :].repeat(n, 1).contiguous()}
    plan = [("ragged", this, None)] + [(name, this, m) for name, m in mutes.items()]
    if "parent" in libs and kind != "auto":
        plan = [("parent", libs["parent"], None)] + plan + [("parent2", libs["parent2"], None)]
    variants = []
    for name, lib, mute in plan:
        rx = make_rx(lib, kind, n, T)
        with B.using(lib):
            res = rx.alloc_result()
            g = B.capture(torch, lambda side, rx=rx, res=res, mute=mute: rx.push(chunk, out=res, lengths=lens, stream=side)
                          if mute is None else rx.push(chunk, out=res, lengths=lens, mute=mute, stream=side))
        variants.append((name, lib, rx, res, g))

    def one_pass(v):
        with B.using(v[1]):
            v[2].reset()
        return [B.timed(torch, v[4]) for _ in range(pushes)]

    # the unmuted variants agree on what they heard, before anything is timed
    ref = None
    for v in variants:
        if v[0] in ("parent", "parent2", "ragged", "mute_none"):
            one_pass(v)
            torch.cuda.synchronize()
            with B.using(v[1]):
                got = (v[3].n_closed.clone(), v[2].busy().clone())
            assert ref is None or (torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])), v[0]
            ref = ref or got
    assert bool(ref[1].any()), "nobody heard the message"
    us = B.rotate(torch, variants, reps, one_pass)
    pairs = [("parent2", "parent"), ("ragged", "parent")] + [(m, "ragged") for m in mutes]
    step = {"stream": "push", "stored": "pushstored", "auto": "pushauto"}[kind]
    base = B.stats(us["ragged"])
    lines.append(f"{step + str(T):9s} {n}x{T}   ragged {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"{base['samples']} pushes of the {kind} receiver)")
    B.report(f"{step}{T}", f"{n}x{T}", us, pairs, lines, results)
    B.close_all(torch, variants)


def carrier(torch, n, T):
    """[n, T] int16: every 64th channel hears a full-scale square wave (its gate opens and stays open), the rest silence."""
    chunk = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    chunk[::64] = torch.tensor([20000, -20000], dtype=torch.int16, device="cuda").repeat(T // 2)
    return chunk


def step_tick(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, DEPTH)
    chunk = carrier(torch, n, T)
    pulled = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    ticks = min(DEPTH * MESSAGE // T, 32)
    variants = {}
    for name in ("hold", "csma"):
        rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=32)
        tx = make_tx(this, n)
        res, ev = rx.alloc_result(), rx.alloc_events(max_events=4096, max_bytes=4096 * 32)
        sub = tx.alloc_submit_result(ev.max_events)
        busy = torch.zeros(n, dtype=torch.int32, device="cuda")

        def tick(side, rx=rx, tx=tx, res=res, ev=ev, sub=sub, busy=busy, csma=name == "csma"):
            rx.push(chunk, out=res, events=ev, stream=side, **(dict(mute=tx.on_air) if csma else {}))
            rx.busy(out=busy, stream=side)
            tx.submit_events(ev, out=sub, stream=side)
            tx.pull(T, out=pulled, hold=busy, holdoff=4800, stream=side, **(dict(persist=63, **CSMA) if csma else {}))

        variants[name] = (rx, tx, busy, B.capture(torch, tick))

    def one_pass(name):
        rx, tx, busy, graph = variants[name]
        rx.reset()
        tx.reset()
        tx.on_air.zero_()
        msgs.submit(this, tx, None)
        torch.cuda.synchronize()
        us = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t0) * 1e6)
        assert int(busy.sum()) == n // 64, (name, "every 64th channel is held")
        return us

    us = {name: [] for name in variants}
    order = list(variants)
    for r in range(reps + 1):
        for i in range(len(order)):
            name = order[(i + r) % len(order)]
            got = one_pass(name)
            if r > 0:
                us[name] += got
    base = B.stats(us["hold"])
    lines.append(f"{'tick' + str(T):9s} {n}x{T}   hold {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"wall clock until the device is done, {base['samples']} ticks)")
    B.report(f"tick{T}", f"{n}x{T} wall", us, [("csma", "hold")], lines, results)
    torch.cuda.synchronize()
    for rx, tx, _, graph in variants.values():
        del graph
        rx.close()
        tx.close()


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": B.Library(_native.LIB_PATH)}
    tmp = None
    if args.parent and not args.step.startswith("tick"):
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = B.Library(args.parent), B.Library(twin)
    lines, results = [], []
    name = args.step.rstrip("0123456789")
    T = int(args.step[len(name):])
    if name == "pull":
        step_pull(torch, libs, args.channels, T, args.reps, lines, results)
    elif name == "tick":
        step_tick(torch, libs, args.channels, T, args.reps, lines, results)
    else:
        step_push(torch, libs, {"push": "stream", "pushstored": "stored", "pushauto": "auto"}[name], args.channels, T,
                  args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_csma_bench.py", runs=[])
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (the unchanged paths are compared against it)")
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
