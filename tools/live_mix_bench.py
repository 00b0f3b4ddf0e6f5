#!/usr/bin/env python3
"""live_mix_bench.py -- what the live medium (afsk_live_mix, live.LiveMedium) costs, against the torch expression it
replaces and against a plain copy, and what its one added include line did to the pull and the push.

    python tools/live_mix_bench.py [--parent PARENT.so] [--plain PLAIN.so] [--channels 65536] [--reps 5] [--json OUT] [--txt OUT]
    python tools/live_mix_bench.py --step mix2048|tick2048|pull8192|push2048 ...    (one step, in this process)

Without --step the tool is a driver shaped like tools/live_csma_bench.py (whose helpers, and those of
tools/live_tx_rated_bench.py, it uses): the steps run one after the other, each as a fresh child process under its own
`timeout`, and the chain stops at the first one that fails -- nothing more is started on the GPU after a fault, an abort
or a time limit.  A step compares all its variants in ONE process over the same buffers: every variant's call is
captured once into a HIP graph and replayed, HIP events around each replay give the time, and the passes take turns.

Steps (n = --channels output rows, T = 2048 or 8192 columns):
  mix     three unity sources per row (station A | station B | a third sender, as LiveMedium.from_matrix([[1, 1]], n,
          extra=1) lays them out)
            torch        out.copy_((a.to(int32) + b.to(int32) + c.to(int32)).clamp(-32768, 32767).to(int16))
            copy         out.copy_(a): one read and one write, the floor
            mix          medium.mix(src, out=out); checked equal to the torch expression before anything is timed
            mix_plain    the same from a build with -DAFSK_LIVE_MIX_PLAIN_ORDER (--plain): blocks in blockIdx order, not
                         through xcd_block
  tick    one graph per tick, wall clock until the device is done: push(events=, mute=on_air) -> busy -> submit_events
          -> pull(out=src rows, hold=busy, persist=63, slot=4800) -> the medium (station + a carrier on every 64th row)
            torch / mix  the medium as the torch expression / as medium.mix
  pull, push   tools/live_csma_bench.py's steps of the same name against --parent (loaded twice: the difference of the
          two copies is the spread identical code shows in this run): the kernels next to the new include line
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

import live_csma_bench as CB  # noqa: E402
import live_tx_rated_bench as B  # noqa: E402
from afskmodem_amd import _native  # noqa: E402
from afskmodem_amd.live import LiveMedium, LiveReceiver  # noqa: E402

SIZES = (2048, 8192)
STEPS = {f"{s}{T}": 300 for s in ("mix", "tick", "pull", "push") for T in SIZES}
REPLAYS = 24                                                  # timed replays per pass


def signal(torch, rows, T, seed):
    """[rows, T] int16 of +-12000 square waves with a seeded phase per row: sums of three clip now and then."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    phase = torch.randint(0, 40, (rows, 1), device="cuda", generator=g, dtype=torch.int16)
    col = (torch.arange(T, device="cuda") % 40).to(torch.int16)[None, :]
    level = torch.tensor([12000, -12000], dtype=torch.int16, device="cuda")
    return torch.where((col + phase) % 40 < 20, level[0], level[1])


def torch_medium(torch, out, parts):
    total = parts[0].to(torch.int32)
    for p in parts[1:]:
        total = total + p.to(torch.int32)
    out.copy_(total.clamp(-32768, 32767).to(torch.int16))


def run_variants(torch, step, shape, variants, reps, pairs, lines, results):
    """variants: [(name, lib, graph, what the graph's launches read and must outlive it)] -> rotate, report."""
    packed = [(name, lib, None, None, g) for name, lib, g, _ in variants]
    us = B.rotate(torch, packed, reps, lambda v: [B.timed(torch, v[4]) for _ in range(REPLAYS)])
    base = B.stats(us[variants[0][0]])
    lines.append(f"{step:9s} {shape:12s} {variants[0][0]} {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"{base['samples']} replays)")
    B.report(step, shape, us, pairs, lines, results)
    torch.cuda.synchronize()
    del packed[:]
    del variants[:]                                             # (the graphs go before the tables they read)


def mediums(libs, build):
    """{"": this build's medium, "_plain": the --plain build's} of ``build()``."""
    out = {}
    for tag, key in (("", "this"), ("_plain", "plain")):
        if key in libs:
            with B.using(libs[key]):
                out[tag] = (libs[key], build())
    return out


def step_mix(torch, libs, n, T, reps, lines, results):
    src = signal(torch, 3 * n, T, 1)
    out = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    a, b, c = src[:n], src[n: 2 * n], src[2 * n:]
    this = libs["this"]
    variants = [("torch", this, B.capture(torch, lambda side: torch_medium(torch, out, (a, b, c))), None),
                ("copy", this, B.capture(torch, lambda side: out.copy_(a)), None)]
    for tag, (lib, m) in mediums(libs, lambda: LiveMedium.from_matrix([[1.0, 1.0]], n, extra=1)).items():
        with B.using(lib):
            variants.append(("mix" + tag, lib, B.capture(torch, lambda side, m=m: m.mix(src, out=out, stream=side)), m))
    variants[0][2].replay()
    torch.cuda.synchronize()
    want = out.clone()
    assert int((want == 32767).sum()) > 0 and int((want == -32768).sum()) > 0, "nothing clips"
    for name, _, g, _ in variants[2:]:
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), (name, "differs from the torch expression")
    del want
    pairs = [("mix", "torch"), ("mix", "copy"), ("torch", "copy"), ("mix_plain", "mix")]
    run_variants(torch, f"mix{T}", f"{n}x{T}", variants, reps, pairs, lines, results)


def step_tick(torch, libs, n, T, reps, lines, results):
    this = libs["this"]
    msgs = B.Messages(torch, n, CB.DEPTH)
    carrier = CB.carrier(torch, n, T)
    ticks = min(CB.DEPTH * CB.MESSAGE // T, 32)
    variants = {}
    for name in ("torch", "mix"):
        rx = LiveReceiver(n, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=32)
        tx = CB.make_tx(this, n)
        res, ev = rx.alloc_result(), rx.alloc_events(max_events=4096, max_bytes=4096 * 32)
        sub = tx.alloc_submit_result(ev.max_events)
        busy = torch.zeros(n, dtype=torch.int32, device="cuda")
        src = torch.zeros((2 * n, T), dtype=torch.int16, device="cuda")         # the station's rows | the carrier's
        src[n:].copy_(carrier)
        chunk = torch.zeros((n, T), dtype=torch.int16, device="cuda")
        medium = LiveMedium.from_matrix([[1.0]], n, extra=1)

        def tick(side, rx=rx, tx=tx, res=res, ev=ev, sub=sub, busy=busy, src=src, chunk=chunk, medium=medium,
                 mix=name == "mix"):
            rx.push(chunk, out=res, events=ev, mute=tx.on_air, stream=side)
            rx.busy(out=busy, stream=side)
            tx.submit_events(ev, out=sub, stream=side)
            tx.pull(T, out=src[:n], hold=busy, holdoff=4800, persist=63, stream=side, **CB.CSMA)
            if mix:
                medium.mix(src, out=chunk, stream=side)
            else:
                with torch.cuda.stream(side):
                    torch_medium(torch, chunk, (src[:n], src[n:]))

        variants[name] = (rx, tx, busy, src, chunk, medium, B.capture(torch, tick))

    def one_pass(name):
        rx, tx, busy, src, chunk, _, graph = variants[name]
        rx.reset()
        tx.reset()
        tx.on_air.zero_()
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
    assert torch.equal(last["torch"], last["mix"]), "the two ticks left different media"
    base = B.stats(us["torch"])
    lines.append(f"{'tick' + str(T):9s} {n}x{T}   torch {base['us_mean']:8.1f} / {base['us_median']:8.1f} us (mean / median, "
                 f"wall clock until the device is done, {base['samples']} ticks)")
    B.report(f"tick{T}", f"{n}x{T} wall", us, [("mix", "torch")], lines, results)
    torch.cuda.synchronize()
    for rx, tx, *_, graph in variants.values():
        del graph
        rx.close()
        tx.close()


def run_step(args):
    import torch
    _native.require_device()
    libs = {"this": B.Library(_native.LIB_PATH)}
    name = args.step.rstrip("0123456789")
    T = int(args.step[len(name):])
    tmp = None
    if args.plain and name == "mix":
        libs["plain"] = B.Library(args.plain)
    if args.parent and name in ("pull", "push"):
        tmp = tempfile.mkdtemp()
        twin = os.path.join(tmp, "libafsk_parent_twin.so")      # a second path: a second copy of the code in the process
        shutil.copy(args.parent, twin)
        libs["parent"], libs["parent2"] = B.Library(args.parent), B.Library(twin)
    lines, results = [], []
    if name == "mix":
        step_mix(torch, libs, args.channels, T, args.reps, lines, results)
    elif name == "tick":
        step_tick(torch, libs, args.channels, T, args.reps, lines, results)
    elif name == "pull":
        CB.step_pull(torch, libs, args.channels, T, args.reps, lines, results)
    else:
        CB.step_push(torch, libs, "stream", args.channels, T, args.reps, lines, results)
    torch.cuda.synchronize()
    if args.json:
        doc = dict(tool="tools/live_mix_bench.py", runs=[])
        if os.path.exists(args.json):
            with open(args.json) as f:
                doc = json.load(f)
        doc["runs"].append(dict(step=args.step, channels=args.channels, reps=args.reps, parent=bool(args.parent),
                                plain=bool(args.plain), results=results))
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
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit (the pull and the push are compared against it)")
    ap.add_argument("--plain", help="libafsk_amd.so of this commit built with -DAFSK_LIVE_MIX_PLAIN_ORDER (the other block order)")
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
        for flag in ("parent", "plain", "json", "txt"):
            if getattr(args, flag):
                cmd += ["--" + flag, getattr(args, flag)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is run", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
