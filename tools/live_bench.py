#!/usr/bin/env python3
"""live_bench.py -- the live receiver (LiveReceiver / afsk_live_push) on synthetic channels, one push per chunk.

    python tools/live_bench.py [--shapes 65536x2048,65536x8192,64x48000] [--seconds 4] [--reps 3] [--json OUT]
                               [--no-verify] [--kernel-stats STATS_CSV]
    python tools/live_bench.py --stream [--stream-cases 65536x8192@1200,...,16384x8192@long] [--json OUT]
    python tools/live_bench.py --tap [--parent PARENT.so] [--tap-cases 65536x8192@1200,...] [--json OUT] [--txt OUT]
    python tools/live_bench.py --ragged [--parent PARENT.so] [--ragged-shape 65536x8192] [--json OUT] [--txt OUT]
    python tools/live_bench.py --events [--shapes ...] [--events-max-burst 96000] [--json OUT] [--txt OUT]
    python tools/live_bench.py --segments [--shapes 65536x8192,65536x2048] [--sparse-every 64] [--json OUT] [--txt OUT]
    python tools/live_bench.py --events | --segments --parent PARENT.so [--shapes ...] [--json OUT] [--txt OUT]

--stream times the stored and the streaming receiver (max_burst_len=None) on the same pushes, alternately, per case
(stream_ab below).  --tap times the streaming receiver's push with and without the payload tap (progressive=True) on the
same pushes, alternately, and -- with --parent, a libafsk_amd.so of the parent commit -- against that build's
streaming push in the same run (tap_ab below).

--ragged times the ragged push and pull (lengths= per channel; ragged_ab below) of the stored, the streaming and the
tapped receiver and of the transmitter against the plain calls, and the plain calls against the parent build's.

--events times what it costs to learn which bursts a push closed (events_ab below): the push alone, the push with the
device-side pack (LiveReceiver.push(events=), afsk_live_pack), and both followed by the host's read -- LiveResult.bursts()
over every slot array against LiveEvents.bursts() over the packed list -- with the bytes each read copies.

--segments times what it costs to put a progressive receiver's payloads together push by push (segments_ab below): the
tapped push alone, the push with the device-side pack (LiveReceiver.push(segments=), afsk_live_pack_tap), and both
followed by the host's PayloadAssembler.feed -- of the result's whole arrays against the packed list -- with the bytes
each copies, on the workload below and on a sparse one where only one channel in --sparse-every carries signal.

--events / --segments with --parent time only the rows of the pack alone (the eager three launches at their densest:
pack_all_slots_us; pack_all_open_us, pack_all_slots_open_us), the parent build's twice and this build's in turn
(pack_alone_ab below).

Per shape (channels x T samples per push, 1200 baud): the channels are synthesized on the device (modulator + oracle
noise at 30 dB, two bursts per channel with payloads of 4 / 12 / 24 bytes at random leads, every eighth channel
silent) into one [channels, seconds * 48000] buffer.  Every push is a column window of that buffer (no copy), captured
once into a HIP graph per window position and replayed; HIP events around each replay give us per push.  Reported:
the median and mean us per push, the audio real-time factor (seconds of audio per channel / wall seconds of the
pushes), and the algorithmic bytes per push over the mean push time as a share of the 8 TB/s HBM peak:
2 B per pushed sample read + 2 B per recorded sample written + the row compaction (read + write) + what the
demodulator must read of every closed burst (bench.py's active samples: up to the squelch-triggering symbol) + the
outputs.  The gate's own bytes (everything but the demodulator's) are printed apart: with --kernel-stats (the
stats CSV of a `rocprofv3 --kernel-trace --stats` run of this tool) the gate kernel's share of peak comes from its
own kernel time.  Unless --no-verify, a seeded sample of channels is checked against Receiver.decode_captures on the
same streams, and every channel's payloads against the transmitted ones.
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import afskmodem_amd as afskmodem  # noqa: E402
from afskmodem_amd import _native, batch, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver  # noqa: E402

PEAK = 8.0e12
BAUD, BF = 1200, 40
PACK_AB_PASSES = 5      # timed passes per variant of the pack-alone rows against --parent
BLOCK = 2048


def walk_bytes(amp, T, n_push, cap_blocks, a_start=18000, a_end=14000):
    """The gate's data movement over the whole stream, from the block amplitudes [n, nb] (the walk of
    live_gate_kernel, vectorised over channels): samples written to the rows and moved by the compaction."""
    n, nb = amp.shape
    mode = np.zeros(n, np.int8)
    rec = np.zeros(n, np.int64)           # blocks recorded in the open burst
    opened_behind = np.zeros(n, bool)     # the open burst opened in this push behind a burst that closed in it
    closed_here = np.zeros(n, bool)
    written = moved = 0
    done = np.array([((b + 1) * BLOCK + T - 1) // T - 1 for b in range(nb)])   # push in which block b completes
    b = 0
    for p in range(n_push):
        # start of push p: the open burst that opened behind closed ones moves to the row front
        moved += int(np.minimum(rec[(mode == 2) & opened_behind], cap_blocks).sum()) * BLOCK
        opened_behind[:] = False
        closed_here[:] = False
        while b < nb and done[b] == p:
            a = amp[:, b]
            m0, m1, m2 = mode == 0, mode == 1, mode == 2
            start = m1 & (a > a_start)
            written += int((start | (m2 & (rec < cap_blocks))).sum()) * BLOCK
            rec = np.where(start, 1, np.where(m2, rec + 1, rec))
            opened_behind |= start & closed_here
            close = m2 & (a < a_end)
            closed_here |= close
            mode = np.where(m0, 1, np.where(start, 2, np.where(close, 0, mode))).astype(np.int8)
            b += 1
    return written, moved


def run_shape(torch, n, T, seconds, reps, verify, seed):
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    samples, sent = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                        silent_every=8, device="cuda")
    max_burst = 48000
    rx = LiveReceiver(n, BF, max_burst_len=max_burst, max_chunk_len=T)
    outs = [rx.alloc_result() for _ in range(2)]
    # eager pass: the bursts, for the checks and the byte count
    got = [[] for _ in range(n)]
    closed_active = 0
    out_bytes = 0
    for p in range(n_push):
        res = rx.push(samples[:, p * T: (p + 1) * T], out=outs[p % 2], flush=p == n_push - 1)
        torch.cuda.synchronize()
        d = res.demod
        active = torch.clamp(torch.clamp(d.term_frame.long() + (d.nbits.long() + 1) * BF, min=4096),
                             max=res.burst_len.reshape(-1).long())
        active = torch.where(res.burst_len.reshape(-1) > 0, active, 0)
        closed_active += int(active.sum())
        out_bytes += int(torch.clamp(d.nbytes, max=d.bytes.shape[1]).sum())
        if verify:
            for c, s, ln, payload in res.bursts():
                got[c].append((s, ln, payload))
    # outputs: the gate's n_closed, burst start / length / flags and the demodulator's slot offset / length; the
    # demodulator's five int32 fields per slot plus the payload bytes
    gate_out = n_push * n * (4 + rx.slots * (8 + 4 + 4 + 8 + 4))
    out_bytes += n_push * n * rx.slots * 20
    # the gate's data movement, from the block amplitudes of the same streams
    nb = total // BLOCK
    g = batch.gate_batch(samples.reshape(-1), torch.arange(n, device="cuda", dtype=torch.int64) * total,
                         torch.full((n,), total, dtype=torch.int32, device="cuda"), total, max_bursts=1, slots=False)
    amp = g.block_amp[:, :nb].cpu().numpy()
    del g
    written, moved = walk_bytes(amp, T, n_push, max_burst // BLOCK)
    gate_bytes = 2 * n * total + 2 * written + 4 * moved + gate_out
    alg_bytes = gate_bytes + 2 * closed_active + out_bytes
    checks = {}
    if verify:
        ok = sum(1 for c in range(n) if [p for _, _, p in got[c]] == [b for _, b in sent[c]])
        checks["roundtrip_channels"] = f"{ok}/{n}"
        rng = np.random.default_rng(seed)
        sample = sorted(rng.choice(n, min(n, 256), replace=False).tolist())
        host = samples[torch.as_tensor(sample, device="cuda")].cpu().numpy()
        want = afskmodem.Receiver(BAUD).decode_captures(list(host), max_bursts=64)
        checks["decode_captures_sample"] = f"{sum(want[j] == [p for _, _, p in got[c]] for j, c in enumerate(sample))}" \
                                           f"/{len(sample)}"
    # graphs: one per column window, replayed in stream order
    rx.reset()
    graphs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p in range(n_push):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=side):
                rx.push(samples[:, p * T: (p + 1) * T], out=outs[p % 2])
            graphs.append(gph)
    torch.cuda.synchronize()
    times = []
    for r in range(reps + 1):
        rx.flush()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_push)]
        for p in range(n_push):
            ev[p][0].record()
            graphs[p].replay()
            ev[p][1].record()
        torch.cuda.synchronize()
        if r:                                          # the first pass warms up
            times += [a.elapsed_time(b) * 1e3 for a, b in ev]
    us = np.asarray(times)
    mean_us = float(us.mean())
    rec = dict(shape=f"{n}x{T}", channels=n, T=T, pushes=n_push, seconds_per_channel=total / 48000, slots=rx.slots,
               us_per_push_median=round(float(np.median(us)), 2), us_per_push_mean=round(mean_us, 2),
               us_per_push_p90=round(float(np.percentile(us, 90)), 2),
               realtime_factor=round((T / 48000) / (mean_us * 1e-6), 1),
               alg_bytes_per_push=int(alg_bytes / n_push), gate_bytes_per_push=int(gate_bytes / n_push),
               recorded_samples=int(written), compaction_samples=int(moved), demod_active_samples=int(closed_active),
               share_of_peak_push=round(alg_bytes / n_push / (mean_us * 1e-6) / PEAK, 3), **checks)
    del graphs, samples
    rx.close()
    torch.cuda.empty_cache()
    return rec


def graphs_for(torch, rx, samples, n_push, T, out):
    """One captured push per column window of `samples`, in stream order."""
    graphs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for p in range(n_push):
            gph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gph, stream=side):
                rx.push(samples[:, p * T: (p + 1) * T], out=out)
            graphs.append(gph)
    torch.cuda.synchronize()
    return graphs


def timed_pass(torch, rx, graphs):
    rx.flush()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in graphs]
    for g, (a, b) in zip(graphs, ev):
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def stream_ab(torch, n, T, seconds, baud, reps, seed, long_messages=False):
    """The stored and the streaming receiver on the same pushes of one workload, timed alternately (stored pass,
    streaming pass, ... after one warm-up pass each).  The synthetic workload is run_shape's at `baud` (stored
    max_burst_len 1 s); long_messages: LiveTransmitter channels with 256-byte payloads back to back at 1200 baud
    (stored max_burst_len 4 s).  The streaming receiver's algorithmic bytes: 2 B per pushed sample + its outputs
    (gate fields and DemodOutputs per slot, the payload bytes) -- it reads no burst a second time."""
    samples, n_push = stream_workload(torch, n, T, seconds, baud, seed, long_messages)
    bf = 48000 // baud
    max_burst = 4 * 48000 if long_messages or bf > 160 else 48000
    stored = LiveReceiver(n, bf, max_burst_len=max_burst, max_chunk_len=T)
    streaming = LiveReceiver(n, bf, max_burst_len=None, max_payload_len=256, max_chunk_len=T)
    # eager pass of both: equal bursts (payloads) wherever the stored receiver holds them
    bursts = []
    for rx in (stored, streaming):
        got = []
        out = rx.alloc_result()
        for p in range(n_push):
            got += rx.push(samples[:, p * T: (p + 1) * T], out=out, flush=p == n_push - 1).bursts()
        bursts.append(got)
    ovf = sum(1 for b in bursts[0] if b[3] == b"" and b[2] > max_burst)
    same = sum(1 for a, b in zip(bursts[0], bursts[1]) if a == b)
    decoded = sum(1 for b in bursts[1] if b[3])
    outs = [stored.alloc_result(), streaming.alloc_result()]
    graphs = [graphs_for(torch, rx, samples, n_push, T, o) for rx, o in zip((stored, streaming), outs)]
    times = [[], []]
    for r in range(reps + 1):
        for i, rx in enumerate((stored, streaming)):
            t = timed_pass(torch, rx, graphs[i])
            if r:
                times[i] += t
    us = [float(np.mean(t)) for t in times]
    slot_out = n * streaming.slots * (8 + 4 + 4 + 20) + n * 4
    pay = sum(len(b[3]) for b in bursts[1])
    alg = 2 * n * T + slot_out + pay / n_push
    rec = dict(shape=f"{n}x{T}", baud=baud, workload="long_messages_256B" if long_messages else "synthetic",
               pushes=n_push, stored_max_burst_len=max_burst,
               stored_state_bytes=stored.state_bytes, streaming_state_bytes=streaming.state_bytes,
               stored_us_mean=round(us[0], 2), streaming_us_mean=round(us[1], 2),
               stored_us_median=round(float(np.median(times[0])), 2),
               streaming_us_median=round(float(np.median(times[1])), 2),
               streaming_over_stored=round(us[1] / us[0], 3),
               streaming_alg_bytes_per_push=int(alg), streaming_share_of_peak=round(alg / (us[1] * 1e-6) / PEAK, 3),
               bursts=len(bursts[1]), streaming_decoded=decoded, equal_to_stored=f"{same}/{len(bursts[0])}",
               stored_overflowed=ovf)
    del graphs, samples
    stored.close()
    streaming.close()
    torch.cuda.empty_cache()
    return rec


def stream_workload(torch, n, T, seconds, baud, seed, long_messages):
    """stream_ab's workload: (samples [n, n_push * T] on the device, n_push)."""
    from afskmodem_amd.live import LiveTransmitter
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    bf = 48000 // baud
    if long_messages:
        tx = LiveTransmitter(n, baud, 0.5, max_payload_len=256)
        rng = np.random.default_rng(seed)
        pays = [bytes(rng.integers(0, 256, 256, dtype=np.uint8)) for _ in range(2 * n)]
        tx.submit(np.repeat(np.arange(n), 2), pays)
        samples = torch.zeros((n, total), dtype=torch.int16, device="cuda")
        samples[:, 4 * BLOCK:] = tx.pull(total - 4 * BLOCK)
        tx.close()
    else:
        plens = (4, 12, 24) if bf <= 160 else (1,)
        samples, _ = synth.live_channels(n, total, baud, seed, bursts_per_channel=2 if bf <= 160 else 1,
                                         payload_lens=plens, silent_every=8, device="cuda")
    return samples, n_push


def load_build(path):
    """Another build of the library (the parent commit's), bound like _native.lib() for the entries it has."""
    L = C.CDLL(path)
    for table in (getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES")):
        for name, (res, args) in table.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
    return L


class using:
    """Route the package's native calls to one build for the duration."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = _native._lib
        if self.lib is not None:
            _native._lib = self.lib

    def __exit__(self, *exc):
        _native._lib = self.saved


def tap_ab(torch, n, T, seconds, baud, reps, seed, long_messages, parent):
    """The streaming push of the parent build (`parent`, a loaded library or None: untapped twice -- the spread of that
    repeat is the margin -- and tapped), this build's untapped push and this build's tapped push (payload rows of 256
    and of 0 bytes) on the same pushes of stream_ab's workload: one
    graph per column window, replayed in stream order with HIP events around each replay; the variants take turns
    pass by pass (after one warm-up pass each), so drift hits all alike.  Per variant: the mean us per push of every
    pass, their mean, and the spread (max - min) / mean of the passes."""
    samples, n_push = stream_workload(torch, n, T, seconds, baud, seed, long_messages)
    bf = 48000 // baud
    variants = ([("parent", parent, {}), ("parent_again", parent, {}), ("parent_tapped", parent, dict(progressive=True))]
                if parent is not None else []) + [
        ("untapped", None, {}), ("tapped", None, dict(progressive=True)),
        ("tapped_rows0", None, dict(progressive=True, max_payload_len=0))]
    runs = []
    for name, lib, kw in variants:
        with using(lib):
            rx = LiveReceiver(n, bf, max_burst_len=None, max_chunk_len=T, **{"max_payload_len": 256, **kw})
            out = rx.alloc_result()
            # eager pass: what the pushes decode (and, tapped, hand out)
            nbytes = tapped = 0
            for p in range(n_push):
                rx.push(samples[:, p * T: (p + 1) * T], out=out, flush=p == n_push - 1)
                nbytes += int(torch.where(out.burst_len.reshape(-1) > 0, out.demod.nbytes, 0).sum())
                tapped += int(out.tap.n.sum()) if out.tap is not None else 0
            graphs = graphs_for(torch, rx, samples, n_push, T, out)
        # (the graphs write into `out`: it lives as long as they do)
        runs.append(dict(name=name, lib=lib, rx=rx, graphs=graphs, out=out, passes=[], nbytes=nbytes, tapped=tapped,
                         tap_cap=rx.tap_cap, state_bytes=rx.state_bytes))
    for r in range(reps + 1):
        for v in runs:
            with using(v["lib"]):
                t = timed_pass(torch, v["rx"], v["graphs"])
            if r:
                v["passes"].append(float(np.mean(t)))
    rec = dict(shape=f"{n}x{T}", baud=baud, workload="long_messages_256B" if long_messages else "synthetic",
               pushes=n_push, reps=reps, variants={})
    for v in runs:
        m = float(np.mean(v["passes"]))
        rec["variants"][v["name"]] = dict(us_mean=round(m, 2), us_passes=[round(x, 2) for x in v["passes"]],
                                          spread=round((max(v["passes"]) - min(v["passes"])) / m, 4),
                                          payload_bytes=v["nbytes"], tap_bytes=v["tapped"], tap_cap=v["tap_cap"],
                                          state_bytes=v["state_bytes"])
    base = rec["variants"].get("parent") or rec["variants"]["untapped"]
    rec["baseline"] = "parent" if "parent" in rec["variants"] else "untapped"
    for name, v in rec["variants"].items():
        v["over_baseline"] = round(v["us_mean"] / base["us_mean"], 4)
    if parent is not None:
        V = rec["variants"]
        a, b = V["parent"]["us_mean"], V["parent_again"]["us_mean"]
        margin = max(abs(a - b) / min(a, b), V["parent"]["spread"], V["parent_again"]["spread"])
        rec["parent_spread"] = round(margin, 4)
        rec["untapped_over_parent"] = round(V["untapped"]["us_mean"] / (0.5 * (a + b)), 4)
        rec["untapped_inside_spread"] = bool(V["untapped"]["us_mean"] <= max(a, b) * (1 + margin))
        rec["tapped_over_parent_tapped"] = round(V["tapped"]["us_mean"] / V["parent_tapped"]["us_mean"], 4)
        rec["tapped_inside_spread"] = bool(V["tapped"]["us_mean"] <= V["parent_tapped"]["us_mean"] * (1 + margin))
    assert len({v["nbytes"] for v in runs}) == 1, "the variants decoded different payloads"
    assert all(v["tapped"] == v["nbytes"] for v in runs if v["tap_cap"]), "the tap byte count is not the sum of nbytes"
    torch.cuda.synchronize()
    for v in runs:
        del v["graphs"], v["out"]
        with using(v["lib"]):
            v["rx"].close()
    del samples
    torch.cuda.empty_cache()
    return rec


def pack_alone_us(torch, pack, reps, parent):
    """Mean us of one eager pack (``pack()``: three launches, HIP events around them) over ``reps`` calls after one
    warm-up call.  With ``parent`` (a loaded library of the parent commit) instead a dict: the variants parent,
    parent_again and this build take turns pass by pass, each pass ``reps`` calls after a warm-up call; the margin is the
    spread between the two parent variants (as tap_ab's), and this build is inside when its mean is at most the mean of
    the two parent variants plus that margin."""
    def one_pass():
        us = []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pack()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        return float(np.mean(us[1:]))

    if parent is None:
        return round(one_pass(), 2)
    variants = (("parent", parent), ("parent_again", parent), ("this", None))
    passes = {name: [] for name, _ in variants}
    for r in range(PACK_AB_PASSES + 1):
        for name, lib in variants:
            with using(lib):
                t = one_pass()
            if r:
                passes[name].append(t)
    V = {name: dict(us_mean=round(float(np.mean(p)), 2), us_passes=[round(x, 2) for x in p],
                    spread=round((max(p) - min(p)) / float(np.mean(p)), 4)) for name, p in passes.items()}
    a, b = V["parent"]["us_mean"], V["parent_again"]["us_mean"]
    margin = max(abs(a - b) / min(a, b), V["parent"]["spread"], V["parent_again"]["spread"])
    return dict(variants=V, margin=round(margin, 4), this_over_parent=round(V["this"]["us_mean"] / (0.5 * (a + b)), 4),
                this_inside_margin=bool(V["this"]["us_mean"] <= 0.5 * (a + b) * (1 + margin)))


def events_pack_alone(torch, rx, o, events, reps, parent, rec):
    """The event pack alone at its densest: every slot of every channel in use with a 24-byte payload (hand-made arrays
    in the result's own tensors; the pack visits a wave's 64 channels one after the other)."""
    o.n_closed.fill_(rx.slots)
    o.flags.zero_()
    o.demod.nbytes.fill_(min(24, int(o.demod.bytes.shape[1])))
    rec["pack_all_slots_us"] = pack_alone_us(torch, lambda: rx.pack(o, out=events), reps, parent)
    rec["pack_all_slots_records"] = int(events.count)


def segments_pack_alone(torch, rx, o, sg, reps, parent, rec):
    """The segment pack alone at its densest, on hand-made arrays in the result's own tensors: every channel with an
    open segment of min(14, tap_cap) bytes (14: what a busy 1200-baud channel decodes in 8192 samples), then every slot
    in use as well (final segments of length 0)."""
    t = o.tap
    k = min(14, rx.tap_cap)
    for name, closed in (("pack_all_open", 0), ("pack_all_slots_open", rx.slots)):
        o.n_closed.fill_(closed)
        o.flags.zero_()
        o.demod.nbytes.fill_(k)
        t.n.fill_(k)
        t.len.zero_()
        t.open_start.fill_(2048)
        t.open_nbytes.fill_(k)
        rec[name + "_us"] = pack_alone_us(torch, lambda: rx.pack_tap(o, out=sg), reps, parent)
        rec[name + "_records"] = int(sg.count)
    rec["pack_all_open_bytes_per_channel"] = k


def pack_alone_ab(torch, n, T, reps, parent, segments, max_burst):
    """--events / --segments with --parent: the pack-alone rows only, this build against the parent's in one process.
    The pack entries take no receiver handle, so one receiver of this build holds the arrays for every variant."""
    if segments:
        rx = LiveReceiver(n, BF, max_burst_len=None, max_payload_len=256, max_chunk_len=T, progressive=True)
        rec = dict(shape=f"{n}x{T}", slots=rx.slots, tap_cap=rx.tap_cap, reps=reps, passes=PACK_AB_PASSES)
        segments_pack_alone(torch, rx, rx.alloc_result(), rx.alloc_segments(), reps, parent, rec)
    else:
        rx = LiveReceiver(n, BF, max_burst_len=max_burst, max_chunk_len=T)
        rec = dict(shape=f"{n}x{T}", slots=rx.slots, out_stride=rx.out_stride, reps=reps, passes=PACK_AB_PASSES)
        events_pack_alone(torch, rx, rx.alloc_result(), rx.alloc_events(), reps, parent, rec)
    torch.cuda.synchronize()
    rx.close()
    torch.cuda.empty_cache()
    return rec


def pack_alone_lines(recs):
    out = ["the pack alone (eager, three launches), us per pack: the parent build twice and this build, taking turns pass "
           "by pass; margin = the larger of the two parent variants' difference and their own spreads"]
    for r in recs:
        for row in [k for k in r if k.endswith("_us")]:
            c, V = r[row], r[row]["variants"]
            out.append(f"{r['shape']:>12s} {row:>24s} {r[row[:-3] + '_records']:9d} records  "
                       + "  ".join(f"{k} {V[k]['us_mean']:8.1f}" for k in ("parent", "parent_again", "this"))
                       + f"  this/parent x{c['this_over_parent']:.4f} (margin {100 * c['margin']:.2f} %: "
                       f"{'inside' if c['this_inside_margin'] else 'OUTSIDE'})")
    return out


def events_ab(torch, n, T, seconds, reps, seed, max_burst):
    """What it costs to learn which bursts a push closed, on run_shape's workload with a stored receiver
    (max_burst_len = max_burst): per push, the variants taking turns pass by pass after one warm-up pass each,
      a  the push alone, replayed from a graph (HIP events around the replay)
      b  push + pack in one graph (likewise)
      c  the replay of a, then LiveResult.bursts() on the host (wall clock from before the replay until the list is there)
      d  the replay of b, then LiveEvents.bursts() on the host (likewise)
    and the bytes c and d copy to the host per push.  c is the path that existed before the pack and the only baseline:
    the spread of its passes, (max - min) / mean, is the margin d's advantage has to exceed."""
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    samples, _ = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                     silent_every=8, device="cuda")
    rx = [LiveReceiver(n, BF, max_burst_len=max_burst, max_chunk_len=T) for _ in range(2)]
    out = [r.alloc_result() for r in rx]
    events = rx[1].alloc_events()
    # eager pass: the packed list reports what the slot arrays report
    n_bursts = payload = 0
    for p in range(n_push):
        w = samples[:, p * T: (p + 1) * T]
        want = rx[0].push(w, out=out[0], flush=p == n_push - 1).bursts()
        got = rx[1].push(w, out=out[1], flush=p == n_push - 1, events=events).events.bursts()
        assert got == want, f"push {p}: the packed list differs from the slot arrays"
        n_bursts += len(want)
        payload += sum(len(b[3]) for b in want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs = [[], []]
    with torch.cuda.stream(side):
        for p in range(n_push):
            for i in range(2):
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=side):
                    rx[i].push(samples[:, p * T: (p + 1) * T], out=out[i], events=events if i else None)
                graphs[i].append(gph)
    torch.cuda.synchronize()
    stride = int(out[0].demod.bytes.shape[1])
    # what LiveResult.bursts() copies, derived from its tensors' sizes (it does not count its copies; LiveEvents does)
    slot_arrays = 4 * n + n * rx[0].slots * 16                     # n_closed; burst_start, burst_len, flags
    demod_arrays = n * rx[0].slots * (stride + 20)                 # the rows and the five vectors (read when a burst closed)

    def host_pass(i):
        rx[i].flush()
        torch.cuda.synchronize()
        us, copied = [], []
        for p in range(n_push):
            t0 = time.perf_counter()
            graphs[i][p].replay()
            got = events.bursts() if i else out[0].bursts()
            us.append((time.perf_counter() - t0) * 1e6)
            copied.append(events.copied_bytes if i else slot_arrays + (demod_arrays if got else 0))
        return us, copied

    passes = dict(a=[], b=[], c=[], d=[])
    per_push = dict(a=[], b=[], c=[], d=[])
    copied = dict(c=[], d=[])
    for r in range(reps + 1):
        for k, i in (("a", 0), ("b", 1)):
            t = timed_pass(torch, rx[i], graphs[i])
            if r:
                passes[k].append(float(np.mean(t)))
                per_push[k] += t
        for k, i in (("c", 0), ("d", 1)):
            t, by = host_pass(i)
            if r:
                passes[k].append(float(np.mean(t)))
                per_push[k] += t
                copied[k] = by
    cell = lambda k: dict(us_mean=round(float(np.mean(per_push[k])), 2),  # noqa: E731
                          us_median=round(float(np.median(per_push[k])), 2),
                          us_passes=[round(x, 2) for x in passes[k]],
                          spread=round((max(passes[k]) - min(passes[k])) / float(np.mean(passes[k])), 4))
    rec = dict(shape=f"{n}x{T}", channels=n, T=T, pushes=n_push, reps=reps, slots=rx[0].slots, out_stride=stride,
               max_burst_len=max_burst, bursts=n_bursts, payload_bytes=payload,
               events_buffer_bytes=int(events.buffer.numel()), push=cell("a"), push_pack=cell("b"),
               push_bursts=cell("c"), push_pack_events=cell("d"),
               host_bytes_per_push_bursts=int(np.mean(copied["c"])), host_bytes_per_push_events=int(np.mean(copied["d"])))
    a, b, c, d = (rec[k]["us_mean"] for k in ("push", "push_pack", "push_bursts", "push_pack_events"))
    rec["pack_us"] = round(b - a, 2)
    rec["pack_over_push"] = round((b - a) / a, 4)
    rec["events_over_bursts"] = round(d / c, 4)
    rec["bursts_spread"] = rec["push_bursts"]["spread"]
    rec["events_faster_beyond_spread"] = bool(d < c * (1 - rec["bursts_spread"]))
    events_pack_alone(torch, rx[1], out[1], events, reps, None, rec)
    del graphs, samples
    torch.cuda.synchronize()
    for r in rx:
        r.close()
    torch.cuda.empty_cache()
    return rec


def events_lines(recs):
    out = ["us per push, mean / median over every push of every timed pass; host bytes copied per push (mean): d bytes are "
           "counted at LiveEvents' copies, c bytes are derived from the sizes of the tensors LiveResult.bursts() copies",
           f"{'shape':>12s} {'bursts':>7s} {'a push':>17s} {'b push+pack':>17s} {'(b-a)/a':>8s} "
           f"{'c push+bursts()':>19s} {'d push+pack+events':>19s} {'d/c':>7s} {'c spread':>9s} "
           f"{'c bytes':>11s} {'d bytes':>9s}"]
    for r in recs:
        f = lambda k, w: f"{r[k]['us_mean']:.1f} / {r[k]['us_median']:.1f}".rjust(w)  # noqa: E731
        out.append(f"{r['shape']:>12s} {r['bursts']:7d} {f('push', 17)} {f('push_pack', 17)} {r['pack_over_push']:8.4f} "
                   f"{f('push_bursts', 19)} {f('push_pack_events', 19)} {r['events_over_bursts']:7.4f} "
                   f"{100 * r['bursts_spread']:8.2f}% {r['host_bytes_per_push_bursts']:11d} "
                   f"{r['host_bytes_per_push_events']:9d}")
    out.append("the pack alone (eager, three launches) with every slot of every channel in use, 24-byte payloads: "
               + ", ".join(f"{r['shape']} {r['pack_all_slots_records']} records {r['pack_all_slots_us']:.1f} us"
                           for r in recs))
    return out


def segments_ab(torch, n, T, seconds, reps, seed, keep_every):
    """What it costs to put a progressive receiver's payloads together push by push, on run_shape's workload
    (keep_every 1: seven channels in eight carry two bursts) or with only one channel in keep_every left and the
    others silent: per push, the variants taking turns pass by pass after one warm-up pass each,
      a  the tapped push alone, replayed from a graph (HIP events around the replay)
      b  push + afsk_live_pack_tap in one graph (likewise)
      c  the replay of a, then PayloadAssembler.feed(result) on the host (wall clock until the bursts are there)
      d  the replay of b, then PayloadAssembler.feed(segments) on the host (likewise)
    and the bytes c and d copy to the host per push.  c is the path that existed before the pack and the only baseline:
    the spread of its passes, (max - min) / mean, is the margin d's difference has to exceed either way."""
    from afskmodem_amd.live import _nbytes
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    samples, _ = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                     silent_every=8, device="cuda")
    if keep_every > 1:
        # (channel 1 of every keep_every: the workload's silent channels are those at multiples of eight)
        samples[torch.arange(n, device="cuda") % keep_every != 1] = 0
    rx = [LiveReceiver(n, BF, max_burst_len=None, max_payload_len=256, max_chunk_len=T, progressive=True)
          for _ in range(2)]
    out = [r.alloc_result() for r in rx]
    sg = rx[1].alloc_segments()
    # eager pass: the packed list is the tap arrays' list, and both assemblers return the same bursts
    asm = [r.assembler() for r in rx]
    n_bursts = payload = n_segments = busy_channels = 0
    for p in range(n_push):
        w = samples[:, p * T: (p + 1) * T]
        res = rx[0].push(w, out=out[0], flush=p == n_push - 1)
        rx[1].push(w, out=out[1], flush=p == n_push - 1, segments=sg)
        parts = res.partials()
        assert sg.partials() == parts, f"push {p}: the packed list differs from the tap arrays"
        want, got = asm[0].feed(res), asm[1].feed(sg)
        assert got == want and asm[0].pending() == asm[1].pending(), f"push {p}: the assemblers differ"
        n_bursts += len(want)
        payload += sum(len(b[3]) for b in want)
        n_segments += len(parts)
        busy_channels += len({e[0] for e in parts})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graphs = [[], []]
    with torch.cuda.stream(side):
        for p in range(n_push):
            for i in range(2):
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=side):
                    rx[i].push(samples[:, p * T: (p + 1) * T], out=out[i], segments=sg if i else None)
                graphs[i].append(gph)
    torch.cuda.synchronize()
    # what feed(result) copies, derived from its tensors' sizes (it does not count its copies; LiveSegments does):
    # partials() -- n_closed, burst_start, nbytes and the five tap tensors -- then n_closed, burst_len, flags, open_start
    o, t = out[0], out[0].tap
    whole = sum(_nbytes(x) for x in (o.n_closed, o.burst_start, o.demod.nbytes, t.bytes, t.n, t.len, t.open_start,
                                     t.open_nbytes, o.n_closed, o.burst_len, o.flags, t.open_start))

    def host_pass(i):
        rx[i].flush()
        torch.cuda.synchronize()
        a = rx[i].assembler()
        us, copied, bursts = [], [], 0
        for p in range(n_push):
            t0 = time.perf_counter()
            graphs[i][p].replay()
            bursts += len(a.feed(sg if i else out[0]))
            us.append((time.perf_counter() - t0) * 1e6)
            copied.append(sg.copied_bytes if i else whole)
        return us, copied, bursts

    passes = dict(a=[], b=[], c=[], d=[])
    per_push = dict(a=[], b=[], c=[], d=[])
    copied = dict(c=[], d=[])
    for r in range(reps + 1):
        for k, i in (("a", 0), ("b", 1)):
            t = timed_pass(torch, rx[i], graphs[i])
            if r:
                passes[k].append(float(np.mean(t)))
                per_push[k] += t
        for k, i in (("c", 0), ("d", 1)):
            t, by, _ = host_pass(i)
            if r:
                passes[k].append(float(np.mean(t)))
                per_push[k] += t
                copied[k] = by
    cell = lambda k: dict(us_mean=round(float(np.mean(per_push[k])), 2),  # noqa: E731
                          us_median=round(float(np.median(per_push[k])), 2),
                          us_passes=[round(x, 2) for x in passes[k]],
                          spread=round((max(passes[k]) - min(passes[k])) / float(np.mean(passes[k])), 4))
    rec = dict(shape=f"{n}x{T}", channels=n, T=T, workload="all" if keep_every <= 1 else f"1_in_{keep_every}",
               signal_fraction=round(1.0 / max(keep_every, 1), 6), pushes=n_push, reps=reps, slots=rx[0].slots,
               tap_cap=rx[0].tap_cap, bursts=n_bursts, payload_bytes=payload,
               segments_per_push=round(n_segments / n_push, 1), busy_channels_per_push=round(busy_channels / n_push, 1),
               segments_buffer_bytes=int(sg.buffer.numel()), push=cell("a"), push_pack=cell("b"),
               push_feed_result=cell("c"), push_pack_feed_segments=cell("d"),
               host_bytes_per_push_result=int(np.mean(copied["c"])), host_bytes_per_push_segments=int(np.mean(copied["d"])))
    a, b, c, d = (rec[k]["us_mean"] for k in ("push", "push_pack", "push_feed_result", "push_pack_feed_segments"))
    rec["pack_us"] = round(b - a, 2)
    rec["pack_over_push"] = round((b - a) / a, 4)
    rec["push_spread"] = rec["push"]["spread"]
    rec["segments_over_result"] = round(d / c, 4)
    rec["result_spread"] = rec["push_feed_result"]["spread"]
    rec["segments_faster_beyond_spread"] = bool(d < c * (1 - rec["result_spread"]))
    rec["segments_slower_beyond_spread"] = bool(d > c * (1 + rec["result_spread"]))
    segments_pack_alone(torch, rx[1], out[1], sg, reps, None, rec)
    del graphs, samples
    torch.cuda.synchronize()
    for r in rx:
        r.close()
    torch.cuda.empty_cache()
    return rec


def segments_lines(recs):
    out = ["us per push, mean / median over every push of every timed pass; host bytes copied per push (mean): d bytes are "
           "counted at LiveSegments' copies, c bytes are derived from the sizes of the tensors feed(result) copies; "
           "workload: all = the tool's channels (7 in 8 carry two bursts), 1_in_K = only one channel in K keeps its signal",
           f"{'shape':>12s} {'workload':>9s} {'seg/push':>9s} {'a push':>17s} {'b push+pack':>17s} {'(b-a)/a':>8s} "
           f"{'a spread':>9s} {'c push+feed(result)':>21s} {'d push+pack+feed(segments)':>27s} {'d/c':>7s} "
           f"{'c spread':>9s} {'c bytes':>10s} {'d bytes':>9s}"]
    for r in recs:
        f = lambda k, w: f"{r[k]['us_mean']:.1f} / {r[k]['us_median']:.1f}".rjust(w)  # noqa: E731
        out.append(f"{r['shape']:>12s} {r['workload']:>9s} {r['segments_per_push']:9.1f} {f('push', 17)} "
                   f"{f('push_pack', 17)} {r['pack_over_push']:8.4f} {100 * r['push_spread']:8.2f}% "
                   f"{f('push_feed_result', 21)} {f('push_pack_feed_segments', 27)} {r['segments_over_result']:7.4f} "
                   f"{100 * r['result_spread']:8.2f}% {r['host_bytes_per_push_result']:10d} "
                   f"{r['host_bytes_per_push_segments']:9d}")
    seen = set()
    dense = []
    for r in recs:
        if r["shape"] not in seen:
            seen.add(r["shape"])
            dense.append(f"{r['shape']} ({r['pack_all_open_bytes_per_channel']} bytes) open only "
                         f"{r['pack_all_open_records']} records {r['pack_all_open_us']:.1f} us, "
                         f"all slots + open {r['pack_all_slots_open_records']} records {r['pack_all_slots_open_us']:.1f} us")
    out.append("the pack alone (eager, three launches; a thread per channel) with an open segment of min(14, tap_cap) bytes "
               "on every channel: " + "; ".join(dense))
    return out


def ragged_windows(torch, samples, lens):
    """The pushes of a ragged schedule as buffers: [P, n, T] where row c of push p holds channel c's next lens[p, c]
    samples of `samples` (and what follows them in the stream beyond: never read)."""
    n, total = samples.shape
    P, T = lens.shape[0], samples.shape[1] // lens.shape[0]
    pos = torch.cumsum(lens.long(), 0) - lens.long()                     # [P, n] first sample of every push
    col = torch.arange(T, device=samples.device)
    return torch.stack([torch.gather(samples, 1, torch.clamp(pos[p][:, None] + col[None, :], max=total - 1))
                        for p in range(P)])


def ragged_ab(torch, n, T, seconds, reps, seed, parent):
    """Per object -- the stored, the streaming and the tapped receiver, the transmitter -- at 1200 baud, every push or
    pull replayed from a captured graph with HIP events around each replay, the variants taking turns pass by pass
    after one warm-up pass each (measuring-on-mi355x, section 5 "Steady state and noise": warm up, compare two
    versions in the same call, alternating them, and measure the spread of a repeat before trusting a difference;
    section 4: call times from device events):
      parent, parent_again  the plain call of the parent build, twice: the spread of that repeat is the margin
      parent_ragged_full    the parent build's ragged call with every length T
      plain                 the plain call of this build (must stay inside the margin of the parent's)
      ragged_full           the ragged call with every length T: what the ragged form itself costs over `plain` (and
                            must stay inside the margin of the parent's)
      ragged_half           the ragged call with lengths drawn uniformly from [T / 2, T] per channel and push: us per
                            call and ns per sample actually taken
    The receivers push stream_ab's synthetic workload (ragged_half: each channel's own consecutive samples, gathered
    per push); the transmitter pulls one 24-byte message per channel, queued before every pass."""
    from afskmodem_amd.live import LiveTransmitter
    samples, n_push = stream_workload(torch, n, T, seconds, BAUD, seed, False)
    rng = np.random.default_rng(seed)
    full = torch.full((n_push, n), T, dtype=torch.int32, device="cuda")
    half = torch.from_numpy(rng.integers(T // 2, T + 1, (n_push, n)).astype(np.int32)).to("cuda")
    half_buf = ragged_windows(torch, samples, half)
    side = torch.cuda.Stream()

    def capture(fn):
        graphs = []
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for p in range(n_push):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    fn(p)
                graphs.append(g)
        torch.cuda.synchronize()
        return graphs

    def timed(graphs):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in graphs]
        for g, (a, b) in zip(graphs, ev):
            a.record()
            g.replay()
            b.record()
        torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) * 1e3 for a, b in ev]))

    window = lambda p: samples[:, p * T: (p + 1) * T]  # noqa: E731
    variants = ([("parent", parent, None), ("parent_again", parent, None), ("parent_ragged_full", parent, full)]
                if parent is not None else []) + [
        ("plain", None, None), ("ragged_full", None, full), ("ragged_half", None, half)]
    rec = dict(shape=f"{n}x{T}", baud=BAUD, pushes=n_push, reps=reps, samples_per_call=dict(
        plain=n * T, ragged_full=n * T, ragged_half=int(half.sum()) // n_push), objects={})
    pay = [bytes(rng.integers(0, 256, 24, dtype=np.uint8)) for _ in range(n)]
    for obj, kw in (("stored", dict(max_burst_len=48000)), ("streaming", dict(max_burst_len=None, max_payload_len=256)),
                    ("tapped", dict(max_burst_len=None, max_payload_len=256, progressive=True)), ("transmitter", None)):
        runs = []
        for name, lib, lens in variants:
            with using(lib):
                if obj == "transmitter":
                    o = LiveTransmitter(n, BAUD, 0.1, max_payload_len=24)
                    buf = torch.zeros((n, T), dtype=torch.int16, device="cuda")
                    graphs = capture((lambda p: o.pull(T, out=buf)) if lens is None else
                                     (lambda p: o.pull(T, out=buf, lengths=lens[p])))
                    keep = buf
                else:
                    o = LiveReceiver(n, BF, max_chunk_len=T, **kw)
                    out = o.alloc_result()
                    src = half_buf if name == "ragged_half" else None
                    graphs = capture((lambda p: o.push(window(p), out=out)) if lens is None else
                                     (lambda p: o.push(window(p) if src is None else src[p], out=out, lengths=lens[p])))
                    keep = out
            runs.append(dict(name=name, lib=lib, o=o, graphs=graphs, keep=keep, passes=[]))
        for r in range(reps + 1):
            for v in runs:
                with using(v["lib"]):
                    if obj == "transmitter":
                        v["o"].reset()
                        v["o"].submit(np.arange(n), pay)
                    else:
                        v["o"].flush()
                    t = timed(v["graphs"])
                if r:
                    v["passes"].append(t)
        cells = {}
        for v in runs:
            m = float(np.mean(v["passes"]))
            cells[v["name"]] = dict(us_mean=round(m, 2), us_passes=[round(x, 2) for x in v["passes"]],
                                    spread=round((max(v["passes"]) - min(v["passes"])) / m, 4))
        if parent is not None:
            a, b = cells["parent"]["us_mean"], cells["parent_again"]["us_mean"]
            margin = max(abs(a - b) / min(a, b), cells["parent"]["spread"], cells["parent_again"]["spread"])
            cells["margin"] = round(margin, 4)
            cells["plain_over_parent"] = round(cells["plain"]["us_mean"] / (0.5 * (a + b)), 4)
            cells["plain_inside_margin"] = bool(cells["plain"]["us_mean"] <= max(a, b) * (1 + margin))
            pr = cells["parent_ragged_full"]["us_mean"]
            cells["ragged_full_over_parent"] = round(cells["ragged_full"]["us_mean"] / pr, 4)
            cells["ragged_full_inside_margin"] = bool(cells["ragged_full"]["us_mean"] <= pr * (1 + margin))
        cells["ragged_full_over_plain"] = round(cells["ragged_full"]["us_mean"] / cells["plain"]["us_mean"], 4)
        cells["ragged_half_over_plain"] = round(cells["ragged_half"]["us_mean"] / cells["plain"]["us_mean"], 4)
        for k in ("plain", "ragged_full", "ragged_half"):
            cells[k]["ns_per_sample_taken"] = round(cells[k]["us_mean"] * 1e3 / rec["samples_per_call"][k], 6)
        rec["objects"][obj] = cells
        torch.cuda.synchronize()
        for v in runs:
            del v["graphs"], v["keep"]
            with using(v["lib"]):
                v["o"].close()
        torch.cuda.empty_cache()
    return rec


def ragged_lines(rec):
    out = [f"{rec['shape']} @{rec['baud']}  {rec['pushes']} calls per pass, {rec['reps']} passes; us per call (mean), "
           f"ns per sample taken"]
    for obj, c in rec["objects"].items():
        cols = [f"{k} {c[k]['us_mean']:9.1f} us" for k in ("parent", "parent_again", "parent_ragged_full", "plain")
                if k in c]
        cols += [f"{k} {c[k]['us_mean']:9.1f} us {c[k]['ns_per_sample_taken']:.5f} ns/sample"
                 for k in ("ragged_full", "ragged_half")]
        tail = f"full/plain x{c['ragged_full_over_plain']:.4f}  half/plain x{c['ragged_half_over_plain']:.4f}"
        if "margin" in c:
            tail += (f"  plain/parent x{c['plain_over_parent']:.4f} (margin {100 * c['margin']:.2f} %: "
                     f"{'inside' if c['plain_inside_margin'] else 'OUTSIDE'})  ragged_full/parent's "
                     f"x{c['ragged_full_over_parent']:.4f} ({'inside' if c['ragged_full_inside_margin'] else 'OUTSIDE'})")
        out.append(f"{obj:12s}" + "  ".join(cols) + "   " + tail)
    return out


def tap_line(rec):
    head = f"{rec['shape']:>11s} @{rec['baud']:<5d} {rec['workload']:19s}"
    cells = [f"{k} {v['us_mean']:8.1f} us x{v['over_baseline']:.4f} (spread {100 * v['spread']:.2f} %)"
             for k, v in rec["variants"].items()]
    tail = ""
    if "parent_spread" in rec:
        word = lambda ok: "inside" if ok else "OUTSIDE"  # noqa: E731
        tail = (f"   parent_spread {100 * rec['parent_spread']:.2f} %: untapped/parent x{rec['untapped_over_parent']:.4f} "
                f"({word(rec['untapped_inside_spread'])}), tapped/parent_tapped x{rec['tapped_over_parent_tapped']:.4f} "
                f"({word(rec['tapped_inside_spread'])})")
    return head + "  ".join(cells) + f"   baseline: {rec['baseline']}" + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x2048,65536x8192,64x48000")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--kernel-stats", help="rocprofv3 --stats kernel CSV of a run of this tool: adds the gate's share")
    ap.add_argument("--results", help="with --kernel-stats: the JSON of the timed run to annotate")
    ap.add_argument("--profiled-shape", help="with --kernel-stats: the one shape the profiled run timed")
    ap.add_argument("--stream", action="store_true",
                    help="stored vs streaming receiver, alternating, per --stream-cases entry (shape@baud, "
                         "shape@long for the LiveTransmitter 256-byte workload)")
    ap.add_argument("--stream-cases", default="65536x8192@1200,65536x2048@1200,65536x8192@12000,65536x8192@300,"
                                              "16384x8192@24,16384x8192@long")
    ap.add_argument("--tap", action="store_true",
                    help="the streaming push with and without the payload tap, alternating, per --tap-cases entry")
    ap.add_argument("--tap-cases", default="65536x8192@1200,65536x2048@1200,16384x8192@long")
    ap.add_argument("--parent", help="with --tap / --ragged: libafsk_amd.so of the parent commit, timed in the same run; "
                                     "with --events / --segments: the pack-alone rows only, against that build's")
    ap.add_argument("--txt", help="with --tap / --ragged: the table as text")
    ap.add_argument("--ragged", action="store_true",
                    help="the ragged push and pull against the plain ones, and the plain ones against --parent")
    ap.add_argument("--ragged-shape", default="65536x8192")
    ap.add_argument("--events", action="store_true",
                    help="the push with and without the device-side pack, and the host's read of the slot arrays "
                         "against its read of the packed list, per --shapes entry")
    ap.add_argument("--events-max-burst", type=int, default=96000,
                    help="with --events: the stored receiver's max_burst_len (default: the receiver's own, 2 s)")
    ap.add_argument("--segments", action="store_true",
                    help="the tapped push with and without the device-side segment pack, and the assembler fed results "
                         "against the assembler fed packed lists, per --shapes entry, dense and sparse")
    ap.add_argument("--sparse-every", type=int, default=64,
                    help="with --segments: the sparse workload keeps the signal of one channel in this many")
    args = ap.parse_args()
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        doc = json.load(open(args.results))
        doc["profiled_shape"] = args.profiled_shape
        for r in rows:
            name = r.get("Name") or r.get("KernelName") or ""
            # the stored sink's instantiations of the push kernel, mangled or demangled (a run pushes through one)
            if "live_push_kernel" in name and "LiveStoreSink" in name:
                doc["gate_kernel_calls"] = int(r["Calls"])
                doc["gate_kernel_mean_us"] = round(float(r["AverageNs"]) / 1e3, 2)
            if "demod_uniform" in name:
                doc.setdefault("demod_kernels", []).append(dict(name=name[:80], calls=int(r["Calls"]),
                                                                 mean_us=round(float(r["AverageNs"]) / 1e3, 2)))
        for rec in doc.get("results", []):
            if "gate_kernel_mean_us" in doc and rec["shape"] == doc.get("profiled_shape"):
                rec["gate_kernel_share_of_peak"] = round(rec["gate_bytes_per_push"] / (doc["gate_kernel_mean_us"] * 1e-6)
                                                         / PEAK, 3)
        print(json.dumps(doc))
        return
    import torch
    res = []
    if (args.events or args.segments) and args.parent:
        parent = load_build(args.parent)
        for shape in args.shapes.split(","):
            n, T = (int(x) for x in shape.split("x"))
            rec = pack_alone_ab(torch, n, T, args.reps, parent, args.segments, args.events_max_burst)
            print(json.dumps(rec), flush=True)
            res.append(rec)
        lines = pack_alone_lines(res)
        print("\n".join(lines))
        mode = "--segments" if args.segments else "--events"
        for path, text in ((args.json, json.dumps(dict(tool=f"tools/live_bench.py {mode} --parent", reps=args.reps,
                                                       results=res), indent=1)),
                           (args.txt, "\n".join(lines) + "\n")):
            if path:
                with open(path, "w") as f:
                    f.write(text)
        return
    if args.events:
        for shape in args.shapes.split(","):
            n, T = (int(x) for x in shape.split("x"))
            rec = events_ab(torch, n, T, args.seconds, args.reps, args.seed, args.events_max_burst)
            print(json.dumps(rec), flush=True)
            res.append(rec)
        lines = events_lines(res)
        print("\n".join(lines))
        for path, text in ((args.json, json.dumps(dict(tool="tools/live_bench.py --events", seconds=args.seconds,
                                                       reps=args.reps, results=res), indent=1)),
                           (args.txt, "\n".join(lines) + "\n")):
            if path:
                with open(path, "w") as f:
                    f.write(text)
        return
    if args.segments:
        for shape in args.shapes.split(","):
            n, T = (int(x) for x in shape.split("x"))
            for keep_every in (1, args.sparse_every):
                rec = segments_ab(torch, n, T, args.seconds, args.reps, args.seed, keep_every)
                print(json.dumps(rec), flush=True)
                res.append(rec)
        lines = segments_lines(res)
        print("\n".join(lines))
        for path, text in ((args.json, json.dumps(dict(tool="tools/live_bench.py --segments", seconds=args.seconds,
                                                       reps=args.reps, sparse_every=args.sparse_every, results=res),
                                                  indent=1)),
                           (args.txt, "\n".join(lines) + "\n")):
            if path:
                with open(path, "w") as f:
                    f.write(text)
        return
    if args.ragged:
        n, T = (int(x) for x in args.ragged_shape.split("x"))
        rec = ragged_ab(torch, n, T, args.seconds, args.reps, args.seed, load_build(args.parent) if args.parent else None)
        lines = ragged_lines(rec)
        print(json.dumps(rec))
        print("\n".join(lines))
        for path, text in ((args.json, json.dumps(dict(tool="tools/live_bench.py --ragged", parent=bool(args.parent),
                                                       seconds=args.seconds, results=[rec]), indent=1)),
                           (args.txt, "\n".join(lines) + "\n")):
            if path:
                with open(path, "w") as f:
                    f.write(text)
        return
    if args.tap:
        parent = load_build(args.parent) if args.parent else None
        lines = []
        for case in args.tap_cases.split(","):
            shape, kind = case.split("@")
            n, T = (int(x) for x in shape.split("x"))
            rec = tap_ab(torch, n, T, args.seconds, 1200 if kind == "long" else int(kind), args.reps, args.seed,
                         kind == "long", parent)
            print(json.dumps(rec), flush=True)
            lines.append(tap_line(rec))
            res.append(rec)
        print("\n".join(lines))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(tool="tools/live_bench.py --tap", parent=bool(args.parent), seconds=args.seconds,
                               reps=args.reps, results=res), f, indent=1)
        if args.txt:
            with open(args.txt, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.stream:
        for case in args.stream_cases.split(","):
            shape, kind = case.split("@")
            n, T = (int(x) for x in shape.split("x"))
            long_messages = kind == "long"
            rec = stream_ab(torch, n, T, args.seconds, 1200 if long_messages else int(kind), args.reps, args.seed,
                            long_messages)
            print(json.dumps(rec), flush=True)
            res.append(rec)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(tool="tools/live_bench.py --stream", seconds=args.seconds, reps=args.reps, results=res),
                          f, indent=1)
        return
    for s in args.shapes.split(","):
        n, T = (int(x) for x in s.split("x"))
        rec = run_shape(torch, n, T, args.seconds, args.reps, not args.no_verify, args.seed)
        print(json.dumps(rec), flush=True)
        res.append(rec)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/live_bench.py", seconds=args.seconds, reps=args.reps, results=res), f, indent=1)


if __name__ == "__main__":
    main()
