#!/usr/bin/env python3
"""live_tx_bench.py -- the live transmitter (LiveTransmitter / afsk_live_tx_pull): one pull per chunk, every channel
kept busy.

    python tools/live_tx_bench.py [--shapes 65536x8192,65536x2048,64x48000] [--steps 24] [--reps 3] [--json OUT]
                                  [--loopback] [--no-verify] [--kernel-stats STATS_CSV --results JSON]

Per shape (channels x T samples per pull, 1200 baud, training 0.5 s, queue depth 4): every channel's queue is
filled with messages of 4 / 12 / 24 / 34 payload bytes and, after every pull, refilled from ``pending`` (up to the
queue depth; outside the timed region), so no channel ever runs idle.  The pull of the fixed T into a fixed
[channels, T] buffer is captured once into a HIP graph and replayed; HIP events around each replay give us per pull.
Reported: the median and mean us per pull, the real-time factor (seconds of audio per channel / wall seconds of a
pull) and the bytes a pull must write (2 B per sample) over the mean pull time as a share of the 8 TB/s HBM peak.
Unless --no-verify, a seeded sample of channels is checked against Transmitter.wav_samples at the starts submit
returned.

--loopback: one graph per chunk of tx.pull into a [channels, T] buffer followed by LiveReceiver.push of the same
buffer; the replays are timed, the refills stop after --steps, the chunks go on until every queue has drained, a flush
ends the streams, and every decoded payload of every channel must equal what was submitted, in order.

--kernel-stats: the stats CSV (or the rocpd database) of a `rocprofv3 --kernel-trace --stats` run of this tool (one
shape); adds the kernels' mean times and the tile kernel's share of peak over the written bytes to the JSON given by
--results.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import afskmodem_amd as afskmodem  # noqa: E402
from afskmodem_amd import _native, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver, LiveTransmitter  # noqa: E402

PEAK = 8.0e12
BAUD, BF, TRAINING = 1200, 40, 0.5
DEPTH = 4
PLENS = np.array([4, 12, 24, 34], np.int32)


class Feeder:
    """Seeded payloads: refill(pending) queues depth - pending messages on every channel and remembers what was
    accepted per channel (for the sample that is verified, or for every channel)."""

    def __init__(self, tx, seed, keep):
        self.tx, self.rng, self.keep = tx, np.random.default_rng(seed), keep
        self.k = 0
        self.sent = {c: [] for c in keep}              # channel -> [(start, payload)]

    def refill(self, pending):
        need = DEPTH - pending
        chans = np.repeat(np.arange(len(need)), need)
        if chans.size == 0:
            return
        plen = self.rng.choice(PLENS, chans.size)
        rows = synth.payload_bytes(self.k, 0, chans.size, int(PLENS.max()))
        self.k += 1
        pays = [rows[i, : plen[i]].tobytes() for i in range(chans.size)]
        res = self.tx.submit(chans, pays)
        if self.keep:
            status, start, _ = res.cpu()
            assert (status == _native.LIVE_TX_QUEUED).all()
            for i in np.nonzero(np.isin(chans, list(self.keep)))[0].tolist():
                self.sent[int(chans[i])].append((int(start[i]), pays[i]))


def render(wav, sent, lo, hi):
    out = np.zeros(hi - lo, np.int16)
    for s, p in sent:
        w = wav(p)
        a, b = max(s, lo), min(s + len(w), hi)
        if a < b:
            out[a - lo: b - lo] = w[a - s: b - s]
    return out


def timed_replays(torch, graph, steps, after):
    us = []
    for k in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
        after(k)
    return us


def capture(torch, fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.synchronize()
    return g


def run_shape(torch, n, T, steps, reps, verify, seed):
    tx = LiveTransmitter(n, BAUD, TRAINING, queue_depth=DEPTH, max_payload_len=int(PLENS.max()))
    rng = np.random.default_rng(seed)
    sample = sorted(rng.choice(n, min(n, 64), replace=False).tolist()) if verify else []
    feed = Feeder(tx, seed, sample)
    feed.refill(np.zeros(n, np.int32))
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    graph = capture(torch, lambda: tx.pull(T, out=buf))
    idx = torch.as_tensor(sample, device="cuda") if sample else None
    got = {c: [] for c in sample}

    def after(k):
        if idx is not None:
            rows = buf[idx].cpu().numpy()
            for j, c in enumerate(sample):
                got[c].append(rows[j])
        feed.refill(tx.pending.cpu().numpy())

    timed_replays(torch, graph, 2, after)                     # warm-up
    us = []
    for _ in range(reps):
        us += timed_replays(torch, graph, steps, after)
    checks = {}
    if verify:
        tr = afskmodem.Transmitter(BAUD, TRAINING)
        cache = {}
        wav = lambda p: cache.setdefault(p, tr.wav_samples(p))  # noqa: E731
        total = T * len(got[sample[0]])
        ok = sum(np.array_equal(np.concatenate(got[c]), render(wav, feed.sent[c], 0, total)) for c in sample)
        checks["verified_channels"] = f"{ok}/{len(sample)}"
    us = np.asarray(us)
    mean_us = float(us.mean())
    written = 2 * n * T
    rec = dict(shape=f"{n}x{T}", channels=n, T=T, pulls=int(us.size), us_per_pull_median=round(float(np.median(us)), 2),
               us_per_pull_mean=round(mean_us, 2), us_per_pull_p90=round(float(np.percentile(us, 90)), 2),
               realtime_factor=round((T / 48000) / (mean_us * 1e-6), 1), written_bytes_per_pull=written,
               share_of_peak_pull=round(written / (mean_us * 1e-6) / PEAK, 3), **checks)
    del graph
    torch.cuda.synchronize()
    tx.close()
    torch.cuda.empty_cache()
    return rec


def run_loopback(torch, n, T, steps, seed):
    tx = LiveTransmitter(n, BAUD, TRAINING, queue_depth=DEPTH, max_payload_len=int(PLENS.max()))
    rx = LiveReceiver(n, BF, max_chunk_len=T)
    feed = Feeder(tx, seed, list(range(n)))
    feed.refill(np.zeros(n, np.int32))
    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
    out = rx.alloc_result()
    graph = capture(torch, lambda: (tx.pull(T, out=buf), rx.push(buf, out=out)))
    got = [[] for _ in range(n)]
    state = dict(k=0, drained=0)

    def after(k):
        for c, _, _, data in out.bursts():
            got[c].append(data)
        pending = tx.pending.cpu().numpy()
        if state["k"] < steps:
            feed.refill(pending)
        state["k"] += 1
        state["drained"] = state["drained"] + 1 if not pending.any() else 0

    us = []
    while state["drained"] < 2:                               # two silent chunks after the last message
        us += timed_replays(torch, graph, 1, after)
    for c, _, _, data in rx.flush().bursts():
        got[c].append(data)
    ok = sum(got[c] == [p for _, p in feed.sent[c]] for c in range(n))
    us = np.asarray(us)
    mean_us = float(us.mean())
    rec = dict(shape=f"{n}x{T}", mode="loopback", channels=n, T=T, chunks=int(us.size),
               us_per_chunk_median=round(float(np.median(us)), 2), us_per_chunk_mean=round(mean_us, 2),
               realtime_factor=round((T / 48000) / (mean_us * 1e-6), 1),
               messages=int(sum(len(v) for v in feed.sent.values())), roundtrip_channels=f"{ok}/{n}")
    del graph
    torch.cuda.synchronize()
    tx.close()
    rx.close()
    torch.cuda.empty_cache()
    return rec


def kernel_rows(stats):
    """(name, calls, total ns) per kernel from a rocprofv3 --stats kernel CSV or a rocpd database (its `kernels` view)."""
    if stats.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(stats)
        return db.execute("select name, count(*), sum(end - start) from kernels group by name").fetchall()
    return [(r.get("Name") or r.get("KernelName") or "", int(r["Calls"]), float(r["TotalDurationNs"]))
            for r in csv.DictReader(open(stats))]


def annotate(stats, results):
    doc = json.load(open(results))
    for name, calls, total_ns in kernel_rows(stats):
        for key, tag in (("tile", "live_tx_tile_kernel"), ("commit", "live_tx_commit_kernel"),
                         ("submit", "live_tx_submit_kernel"), ("order", "live_tx_order_kernel")):
            if tag in name:
                k = doc.setdefault("kernels", {}).setdefault(key, dict(calls=0, total_ns=0.0))
                k["calls"] += int(calls)
                k["total_ns"] += float(total_ns)
    for k in doc.get("kernels", {}).values():
        k["mean_us"] = round(k["total_ns"] / max(k["calls"], 1) / 1e3, 2)
    tile = doc.get("kernels", {}).get("tile")
    for rec in doc.get("results", []):
        if tile and "written_bytes_per_pull" in rec:
            rec["tile_kernel_mean_us"] = tile["mean_us"]
            rec["tile_kernel_share_of_peak"] = round(rec["written_bytes_per_pull"] / (tile["mean_us"] * 1e-6) / PEAK, 3)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x8192,65536x2048,64x48000")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--loopback", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--results")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(annotate(args.kernel_stats, args.results)))
        return
    import torch
    _native.require_device()
    res = []
    for s in args.shapes.split(","):
        n, T = (int(x) for x in s.split("x"))
        if args.loopback:
            rec = run_loopback(torch, n, T, args.steps, args.seed)
        else:
            rec = run_shape(torch, n, T, args.steps, args.reps, not args.no_verify, args.seed)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/live_tx_bench.py", loopback=args.loopback, steps=args.steps, reps=args.reps,
                           results=res), f, indent=1)


if __name__ == "__main__":
    main()
