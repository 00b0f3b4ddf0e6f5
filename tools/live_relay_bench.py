#!/usr/bin/env python3
"""live_relay_bench.py -- one relay tick on the device against the same tick through the host.

    python tools/live_relay_bench.py [--channels 65536] [--chunks 2048,8192] [--seconds 2] [--reps 3]
                                     [--txt profiles/live_relay_bench.txt] [--json OUT]

A relay station hears n channels and answers on n channels: every burst a push closes is queued on the transmitter
channel of the same number, and every tick pulls the next T samples of what is to be sent.  The workload is that of
tools/live_bench.py at 1200 baud (synth.live_channels: two bursts per channel with payloads of 4 / 12 / 24 bytes at
random leads, noise at 30 dB, every eighth channel silent), heard by a streaming receiver.  Per T, over the same sample
buffer and in one process, the two ticks take turns pass by pass (a pass is every tick of the buffer, in stream order,
after one warm-up pass each; receiver and transmitter are reset before a pass):

  graph     push(events=) -> submit_events(out=) -> pull, captured once per column window into ONE graph and replayed;
            wall clock from before the replay until the device has finished, and the device time between HIP events
            around the replay
  host hop  push(events=) -> events.bursts() (a synchronise and the copy of the packed list to the host) ->
            LiveTransmitter.submit of the non-empty payloads (one upload) -> pull, as eager calls; wall clock from
            before the push until the device has finished

and a checking pass compares what the two transmitters sent, tick by tick.  Then submit_events alone (eager, its two
launches between HIP events, the transmitter reset before every call) over hand-made push outputs: a burst of 24 bytes
in the first slot of one channel in 1024, and one in every slot of every channel.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from afskmodem_amd import _native, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver, LiveTransmitter  # noqa: E402

BAUD, BF = 1200, 40


def station(n, T):
    rx = LiveReceiver(n, BF, max_burst_len=None, max_payload_len=256, max_chunk_len=T)
    tx = LiveTransmitter(n, BAUD, 0.1, queue_depth=4, max_payload_len=256)
    return rx, tx, rx.alloc_result(), rx.alloc_events()


def relay_ab(torch, n, T, seconds, reps, seed):
    total = int(seconds * 48000) // T * T
    n_push = total // T
    samples, _ = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                     silent_every=8, device="cuda")
    window = lambda p: samples[:, p * T: (p + 1) * T]  # noqa: E731
    g_rx, g_tx, g_res, g_ev = station(n, T)
    h_rx, h_tx, h_res, h_ev = station(n, T)
    g_sub = g_tx.alloc_submit_result(g_ev.max_events)
    g_out, h_out = (torch.zeros((n, T), dtype=torch.int16, device="cuda") for _ in range(2))

    def host_tick(p):
        h_rx.push(window(p), out=h_res, events=h_ev)
        heard = [(c, data) for c, _, _, data in h_ev.bursts() if data]
        if heard:
            h_tx.submit([c for c, _ in heard], [d for _, d in heard])
        h_tx.pull(T, out=h_out)
        return len(heard)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs = []
    with torch.cuda.stream(side):
        for p in range(n_push):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                g_rx.push(window(p), out=g_res, events=g_ev, stream=side)
                g_tx.submit_events(g_ev, out=g_sub, stream=side)
                g_tx.pull(T, out=g_out, stream=side)
            graphs.append(g)
    torch.cuda.synchronize()

    def restart():
        for rx, tx in ((g_rx, g_tx), (h_rx, h_tx)):
            rx.reset()
            tx.reset()
        torch.cuda.synchronize()

    # the checking pass: both stations send the same samples, tick by tick
    restart()
    relayed = queued = same = sent_ticks = 0
    for p in range(n_push):
        graphs[p].replay()
        relayed += host_tick(p)
        torch.cuda.synchronize()
        queued += int((g_sub.status == _native.LIVE_TX_QUEUED).sum())
        same += int(torch.equal(g_out, h_out))
        sent_ticks += int(g_out.any())

    wall = dict(graph=[], host=[])
    device = []
    passes = dict(graph=[], host=[])
    for r in range(reps + 1):
        restart()
        t_pass = []
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_push)]
        for p in range(n_push):
            t0 = time.perf_counter()
            ev[p][0].record()
            graphs[p].replay()
            ev[p][1].record()
            torch.cuda.synchronize()
            t_pass.append((time.perf_counter() - t0) * 1e6)
        if r:
            wall["graph"] += t_pass
            passes["graph"].append(float(np.mean(t_pass)))
            device += [a.elapsed_time(b) * 1e3 for a, b in ev]
        t_pass = []
        for p in range(n_push):
            t0 = time.perf_counter()
            host_tick(p)
            torch.cuda.synchronize()
            t_pass.append((time.perf_counter() - t0) * 1e6)
        if r:
            wall["host"] += t_pass
            passes["host"].append(float(np.mean(t_pass)))
    cell = lambda k: dict(us_mean=round(float(np.mean(wall[k])), 1),  # noqa: E731
                          us_median=round(float(np.median(wall[k])), 1),
                          us_p90=round(float(np.percentile(wall[k], 90)), 1),
                          us_passes=[round(x, 1) for x in passes[k]],
                          spread=round((max(passes[k]) - min(passes[k])) / float(np.mean(passes[k])), 4))
    rec = dict(shape=f"{n}x{T}", channels=n, T=T, ticks=n_push, reps=reps, slots=g_rx.slots,
               bursts_relayed_host=relayed, bursts_queued_graph=queued, ticks_with_equal_samples=f"{same}/{n_push}",
               ticks_that_send=sent_ticks, graph=cell("graph"), host_hop=cell("host"),
               graph_device_us_mean=round(float(np.mean(device)), 1),
               graph_device_us_median=round(float(np.median(device)), 1))
    rec["graph_over_host_hop"] = round(rec["graph"]["us_mean"] / rec["host_hop"]["us_mean"], 4)
    rec["host_hop_spread"] = rec["host_hop"]["spread"]
    rec["graph_faster_beyond_spread"] = bool(rec["graph"]["us_mean"]
                                             < rec["host_hop"]["us_mean"] * (1 - rec["host_hop_spread"]))
    del graphs
    torch.cuda.synchronize()
    for x in (g_rx, g_tx, h_rx, h_tx):
        x.close()
    del samples
    torch.cuda.empty_cache()
    return rec


def submit_alone(torch, n, T, reps):
    """submit_events alone over hand-made push outputs in a result's own tensors."""
    rx, tx, res, ev = station(n, T)
    sub = tx.alloc_submit_result(ev.max_events)
    d = res.demod
    d.status.zero_()
    d.nbytes.fill_(24)
    d.bytes.copy_(torch.randint(0, 256, tuple(d.bytes.shape), dtype=torch.uint8, device="cuda"))
    res.flags.zero_()
    out = {}
    for name, fill in (("few", None), ("all", rx.slots)):
        res.n_closed.zero_()
        if fill is None:
            res.n_closed[::1024] = 1
        else:
            res.n_closed.fill_(fill)
        rx.pack(res, out=ev)
        us = []
        for _ in range(10 * reps + 1):
            tx.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tx.submit_events(ev, out=sub)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        status = sub.status.cpu().numpy()
        out[name] = dict(records=int(ev.count), queued=int((status == _native.LIVE_TX_QUEUED).sum()),
                         us_mean=round(float(np.mean(us[1:])), 1), us_median=round(float(np.median(us[1:])), 1),
                         us_min=round(float(np.min(us[1:])), 1))
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    torch.cuda.empty_cache()
    return dict(shape=f"{n}x{T}", slots=rx.slots, max_events=ev.max_events, payload_bytes=24, **out)


def lines_of(ticks, alone):
    out = ["one relay tick, us (wall clock until the device has finished; mean / median / p90 over every tick of every "
           "timed pass); the two ticks take turns pass by pass over the same buffer",
           f"{'shape':>12s} {'ticks':>6s} {'relayed':>8s} {'graph tick':>26s} {'graph, device':>15s} "
           f"{'host-hop tick':>26s} {'graph/host':>11s} {'host spread':>12s} {'same samples':>13s}"]
    for r in ticks:
        f = lambda k: f"{r[k]['us_mean']:.1f} / {r[k]['us_median']:.1f} / {r[k]['us_p90']:.1f}".rjust(26)  # noqa: E731
        out.append(f"{r['shape']:>12s} {r['ticks']:6d} {r['bursts_queued_graph']:8d} {f('graph')} "
                   f"{r['graph_device_us_mean']:15.1f} {f('host_hop')} {r['graph_over_host_hop']:11.4f} "
                   f"{100 * r['host_hop_spread']:11.2f}% {r['ticks_with_equal_samples']:>13s}")
    out.append("submit_events alone (eager, two launches between HIP events), us mean / median / min:")
    for r in alone:
        for k in ("few", "all"):
            c = r[k]
            out.append(f"{r['shape']:>12s} {k:>4s}: {c['records']:7d} records, {c['queued']:7d} queued "
                       f"{c['us_mean']:9.1f} / {c['us_median']:.1f} / {c['us_min']:.1f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--chunks", default="2048,8192")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--txt", default=os.path.join("profiles", "live_relay_bench.txt"))
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    ticks, alone = [], []
    for T in (int(x) for x in args.chunks.split(",")):
        rec = relay_ab(torch, args.channels, T, args.seconds, args.reps, args.seed)
        print(json.dumps(rec), flush=True)
        ticks.append(rec)
        rec = submit_alone(torch, args.channels, T, args.reps)
        print(json.dumps(rec), flush=True)
        alone.append(rec)
    lines = lines_of(ticks, alone)
    print("\n".join(lines))
    for path, text in ((args.txt, "\n".join(lines) + "\n"),
                       (args.json, json.dumps(dict(tool="tools/live_relay_bench.py", seconds=args.seconds,
                                                   reps=args.reps, ticks=ticks, submit_alone=alone), indent=1))):
        if path:
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
