#!/usr/bin/env python3
"""live_mixed_bench.py -- the live receiver and transmitter with a rate per channel, against the same objects at one
rate, in one process.

    python tools/live_mixed_bench.py [--shapes 65536x8192,65536x2048] [--seconds 4] [--steps 24] [--reps 3]
                                     [--only push,pull,loopback] [--uniform-baud 1200] [--json OUT]

Per shape (channels x T samples per chunk) and per rate set -- "uniform": 1200 baud everywhere; "mixed": 300 / 600 /
1200 / 2400 baud interleaved channel by channel (channel c at rate c % 4); --uniform-baud sets the one rate of the
"uniform" set (where the mixed set's time goes: its rates one at a time) -- every operation is captured once into a
HIP graph and replayed; HIP events around each replay give us per operation.

push      synth.live_channels captures of each channel's rate (two bursts of 4 / 12 / 24 bytes, training 0.25 s, every
          eighth channel silent, 30 dB) in one [channels, seconds * 48000] buffer; one graph per column window.  The
          bytes a push moves: 2 B per pushed sample read, 2 B per recorded sample written (tools/live_bench.walk_bytes),
          2 B per sample the demodulator must read of every closed burst (up to the squelch-triggering symbol, at the
          slot's own rate: fewer than a 1200-baud burst's at 2400 baud, more at 300), and the outputs.
pull      every channel's queue kept full (depth 4, payloads of 4 / 12 / 24 / 34 bytes, training 0.5 s; refilled outside
          the timed region); the bytes a pull moves: 2 B per written sample.
loopback  tx.pull into a [channels, T] buffer then rx.push of it, captured as one graph and replayed for every chunk
          until the queues (two messages per channel) have drained; every payload must come back.

The share of the 8 TB/s HBM peak is over those bytes and the mean time.  The ratio lines compare the mixed set to the
uniform one of the same run (the issue's aims: push <= 1.15x, pull <= 1.10x).
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from afskmodem_amd import _native, batch, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver, LiveTransmitter  # noqa: E402
from live_bench import walk_bytes  # noqa: E402

PEAK = 8.0e12
MIXED_BAUDS = (300, 600, 1200, 2400)
BLOCK = 2048
MAX_BURST = 96000            # a 300-baud burst of 24 bytes is ~71000 samples


UNIFORM_BAUD = [1200]


def bauds_for(kind, n):
    return np.full(n, UNIFORM_BAUD[0]) if kind == "uniform" else np.asarray([MIXED_BAUDS[c % 4] for c in range(n)])


def rates_arg(kind, values, scalar):
    """The constructor's rate argument: the per-channel list of a mixed set, the scalar of a uniform one."""
    return values.tolist() if kind == "mixed" else scalar


def stats(us):
    us = np.asarray(us)
    return dict(us_median=round(float(np.median(us)), 2), us_mean=round(float(us.mean()), 2),
                us_p90=round(float(np.percentile(us, 90)), 2))


def replay_timed(torch, graphs, reps, before=None):
    """Replay graphs[0..] in order reps + 1 times (the first warms up); us per replay."""
    times = []
    for r in range(reps + 1):
        if before:
            before()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in graphs]
        for g, (a, b) in zip(graphs, ev):
            a.record()
            g.replay()
            b.record()
        torch.cuda.synchronize()
        if r:
            times += [a.elapsed_time(b) * 1e3 for a, b in ev]
    return times


def captures(torch, bauds, total, seed):
    n = len(bauds)
    data = torch.empty((n, total), dtype=torch.int16, device="cuda")
    for j, b in enumerate(sorted(set(bauds.tolist()))):
        idx = np.nonzero(bauds == b)[0]
        s, _ = synth.live_channels(len(idx), total, int(b), seed + j, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                   silent_every=8, device="cuda")
        data[torch.from_numpy(idx).cuda()] = s
        del s
    return data


def bench_push(torch, kind, n, T, seconds, reps, seed):
    bauds = bauds_for(kind, n)
    bf = (48000 // bauds).astype(np.int32)
    n_push = int(seconds * 48000) // T
    total = n_push * T
    data = captures(torch, bauds, total, seed)
    rx = LiveReceiver(n, rates_arg(kind, bf, int(bf[0])), max_burst_len=MAX_BURST, max_chunk_len=T)
    outs = [rx.alloc_result() for _ in range(2)]
    slot_bf = torch.from_numpy(np.repeat(bf, rx.slots).astype(np.int64)).cuda()
    active = out_bytes = 0
    for p in range(n_push):                               # eager pass: the bytes the demodulator reads
        res = rx.push(data[:, p * T: (p + 1) * T], out=outs[p % 2], flush=p == n_push - 1)
        d = res.demod
        bl = res.burst_len.reshape(-1).long()
        a = torch.clamp(torch.clamp(d.term_frame.long() + (d.nbits.long() + 1) * slot_bf, min=4096), max=bl)
        active += int(torch.where(bl > 0, a, 0).sum())
        out_bytes += int(torch.clamp(d.nbytes, max=d.bytes.shape[1]).sum())
    out_bytes += n_push * n * (4 + rx.slots * (8 + 4 + 4 + 8 + 4 + 20))
    g = batch.gate_batch(data.reshape(-1), torch.arange(n, device="cuda", dtype=torch.int64) * total,
                         torch.full((n,), total, dtype=torch.int32, device="cuda"), total, max_bursts=1, slots=False)
    amp = g.block_amp[:, : total // BLOCK].cpu().numpy()
    del g
    written, moved = walk_bytes(amp, T, n_push, MAX_BURST // BLOCK)
    moved_bytes = 2 * n * total + 2 * written + 4 * moved + 2 * active + out_bytes
    rx.reset()
    graphs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p in range(n_push):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=side):
                rx.push(data[:, p * T: (p + 1) * T], out=outs[p % 2])
            graphs.append(gph)
    torch.cuda.synchronize()
    us = replay_timed(torch, graphs, reps, before=rx.flush)
    rec = dict(op="push", rates=kind, shape=f"{n}x{T}", pushes=n_push, slots=rx.slots, **stats(us),
               bytes_per_push=int(moved_bytes / n_push), demod_active_samples=int(active))
    rec["share_of_peak"] = round(rec["bytes_per_push"] / (rec["us_mean"] * 1e-6) / PEAK, 3)
    del graphs, data
    rx.close()
    torch.cuda.empty_cache()
    return rec


def refill(tx, rng, depth, k):
    need = depth - tx.pending.cpu().numpy()
    chans = np.repeat(np.arange(len(need)), need)
    if chans.size:
        plen = rng.choice(np.array([4, 12, 24, 34]), chans.size)
        rows = synth.payload_bytes(k, 0, chans.size, 34)
        tx.submit(chans, [rows[i, : plen[i]].tobytes() for i in range(chans.size)])
    torch_sync()


def torch_sync():
    import torch
    torch.cuda.synchronize()


def bench_pull(torch, kind, n, T, steps, reps, seed):
    bauds = bauds_for(kind, n)
    depth = 4
    tx = LiveTransmitter(n, rates_arg(kind, bauds, int(bauds[0])), 0.5, queue_depth=depth, max_payload_len=34)
    rng = np.random.default_rng(seed)
    buf = torch.empty((n, T), dtype=torch.int16, device="cuda")
    refill(tx, rng, depth, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tx.pull(T, out=buf)
    torch.cuda.synchronize()
    us = []
    for k in range(reps * steps + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        if k >= steps:
            us.append(a.elapsed_time(b) * 1e3)
        refill(tx, rng, depth, k + 1)
    rec = dict(op="pull", rates=kind, shape=f"{n}x{T}", pulls=len(us), **stats(us), bytes_per_pull=2 * n * T)
    rec["share_of_peak"] = round(rec["bytes_per_pull"] / (rec["us_mean"] * 1e-6) / PEAK, 3)
    del graph
    tx.close()
    torch.cuda.empty_cache()
    return rec


def bench_loopback(torch, kind, n, T, seed):
    bauds = bauds_for(kind, n)
    rng = np.random.default_rng(seed)
    tx = LiveTransmitter(n, rates_arg(kind, bauds, int(bauds[0])), 0.25, queue_depth=2, max_payload_len=16)
    rx = LiveReceiver(n, rates_arg(kind, 48000 // bauds, 48000 // int(bauds[0])), max_burst_len=MAX_BURST,
                      max_chunk_len=T)
    plen = rng.integers(0, 17, 2 * n)
    rows = synth.payload_bytes(seed, 0, 2 * n, 16)
    pays = [rows[i, : plen[i]].tobytes() for i in range(2 * n)]
    res = tx.submit(np.repeat(np.arange(n), 2), pays)
    last_end = int((res.start + res.n_samples.to(torch.int64)).max().item())
    n_chunks = -(-(last_end + 2 * BLOCK) // T)
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    out = rx.alloc_result()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tx.pull(T, out=buf)
            rx.push(buf, out=out)
    torch.cuda.synchronize()
    got = [[] for _ in range(n)]
    us = []
    for _ in range(n_chunks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
        for c, _, _, data in out.bursts():
            got[c].append(data)
    for c, _, _, data in rx.flush().bursts():
        got[c].append(data)
    ok = sum(got[c] == pays[2 * c: 2 * c + 2] for c in range(n))
    rec = dict(op="loopback", rates=kind, shape=f"{n}x{T}", chunks=n_chunks, **stats(us),
               roundtrip_channels=f"{ok}/{n}")
    del graph
    tx.close()
    rx.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x8192,65536x2048")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--only", default="push,pull,loopback")
    ap.add_argument("--uniform-baud", type=int, default=1200)
    ap.add_argument("--json")
    args = ap.parse_args()
    UNIFORM_BAUD[0] = args.uniform_baud
    import torch
    _native.require_device()
    ops = args.only.split(",")
    res = []
    for s in args.shapes.split(","):
        n, T = (int(x) for x in s.split("x"))
        for op in ops:
            recs = {}
            for kind in ("uniform", "mixed"):
                if op == "push":
                    r = bench_push(torch, kind, n, T, args.seconds, args.reps, args.seed)
                elif op == "pull":
                    r = bench_pull(torch, kind, n, T, args.steps, args.reps, args.seed)
                else:
                    r = bench_loopback(torch, kind, n, T, args.seed)
                print(json.dumps(r), flush=True)
                res.append(r)
                recs[kind] = r
            ratio = dict(op=op, shape=s, uniform_baud=args.uniform_baud, mixed_over_uniform_mean=round(recs["mixed"]["us_mean"] / recs["uniform"]["us_mean"], 3),
                         mixed_over_uniform_median=round(recs["mixed"]["us_median"] / recs["uniform"]["us_median"], 3))
            print(json.dumps(ratio), flush=True)
            res.append(ratio)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/live_mixed_bench.py", seconds=args.seconds, reps=args.reps,
                           uniform_baud=args.uniform_baud, results=res), f, indent=1)


if __name__ == "__main__":
    main()
