#!/usr/bin/env python3
"""detect_bench.py -- what detecting the rates of a batch costs, against what a user without a detector must do.

    python tools/detect_bench.py [--streams 65536] [--reps 10] [--rounds 3] [--txt OUT] [--json OUT]

One batch: ``--streams`` x 1 s streams of the config-3 mix (300 / 1200 / 2400 baud cycling per stream, training 0.5 s,
a one-second payload, .wav samples; bench.py's config3 generator settings), modulated on the device.  On that batch,
in one process, HIP events around ``--reps`` back-to-back launches, ``--rounds`` rounds that run the variants one after
the other (the median over rounds is reported, with the spread):

  detect K          ``batch.detect_rates`` with K = 1, 4, 18 and 36 candidates (K = 1: [40]; 4: [160, 40, 20, 4]; 18: every
                    other value of VALID_BIT_FRAMES, which holds the three true rates; 36: all)
  demod mixed       ONE ``demod_batch`` through the per-stream entry with the TRUE rates in device memory -- the pass a
                    user makes once the rates are known
  K x demod uniform K uniform ``demod_batch`` launches over the whole batch, one per candidate rate -- what finding the
                    rate costs today (demodulate at every candidate, keep what decoded)
  chain             detect 36 + demod mixed with the DETECTED rates

Reported: the times, detect K / (K uniform passes), detect K / one mixed pass, and the detector's LDS read rate -- the
bytes its seven prefix-sum reads per offset and per cycle start fetch, over the time, against the chip's aggregate
ds_read_b32 rate of about 75 TB/s.  The run also checks that the 36-candidate detection names every stream's true rate.
A 1 s stream is 96 KB of which the detector reads 8 KB; at 65536 streams that is 512 MiB, twice the Infinity Cache.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from afskmodem_amd import _native, batch, synth  # noqa: E402

STREAM_LEN = 48000
BAUDS = (300, 1200, 2400)
LDS_PEAK = 75e12          # aggregate ds_read_b32, bytes / s


def candidates_for(k):
    v = batch.VALID_BIT_FRAMES
    return {1: [40], 4: [160, 40, 20, 4], 18: list(v[1::2]), 36: list(v)}[k]


def lds_bytes(cands, true_bf):
    """Bytes the candidate loops read from LDS for one stream: 7 dwords per offset, and per cycle start from the
    clock index on (the clock index taken as 0: an upper bound within one cycle's worth of reads)."""
    total = 0
    for bf in cands:
        n_off = 4096 - 2 * bf
        total += 28 * (n_off + (n_off - 1) // (2 * bf) + 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--txt")
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    _native.require_device()
    dev = torch.device("cuda", 0)
    n = args.streams
    baud = np.asarray([BAUDS[i % 3] for i in range(n)], np.int32)
    bf_h = (48000 // baud).astype(np.int32)
    plen = np.asarray([synth.one_second_payload(int(b)) for b in baud], np.int32)
    payload = synth.payload_bytes(5, 0, n, int(plen.max()))
    ts = np.asarray([synth.ts_cycles_for(int(b)) for b in baud], np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    samples = torch.empty(n * STREAM_LEN, dtype=torch.int16, device=dev)
    off, ln = batch.uniform_layout(n, STREAM_LEN, dev)
    d_bf = t(bf_h)
    batch.modulate_batch(t(payload), t(plen), d_bf, t(ts), off, ln, STREAM_LEN, samples, True)
    torch.cuda.synchronize()
    stride = batch.out_stride_for(STREAM_LEN, 4)          # (rows that hold any candidate's output)
    out = batch.alloc_result(n, stride, dev)
    ks = (1, 4, 18, 36)
    rate_out = {k: batch.detect_rates(samples, off, ln, candidates_for(k)) for k in ks}
    torch.cuda.synchronize()
    found = rate_out[36].cpu()
    wrong = int((found.bit_frames != bf_h).sum())
    gap = int((found.runner_up - found.score).min())

    variants = {}
    for k in ks:
        variants[f"detect {k}"] = (lambda k=k: batch.detect_rates(samples, off, ln, candidates_for(k), out=rate_out[k]))
    variants["demod mixed"] = lambda: batch.demod_batch(samples, off, ln, d_bf, out=out, entry="mixed")
    for k in ks:
        def passes(k=k):
            for bf in candidates_for(k):
                batch.demod_batch(samples, off, ln, int(bf), out=out, entry="uniform")
        variants[f"{k} x demod uniform"] = passes

    def chain():
        batch.detect_rates(samples, off, ln, None, out=rate_out[36])
        batch.demod_batch(samples, off, ln, rate_out[36].bit_frames, out=out, entry="mixed")
    variants["chain detect 36 + demod mixed"] = chain

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps                    # ms per call

    for fn in variants.values():                           # warm-up: every variant once
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            reps = args.reps if "x demod" not in name else max(1, args.reps // 4)
            ms[name].append(timed(fn, reps))
    chained = out.payloads()
    decoded = sum(chained[s] == payload[s, : plen[s]].tobytes() for s in range(min(n, 4096)))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines = [f"detect_bench: {n} x 1 s streams, config-3 mix (300 / 1200 / 2400 baud), {torch.cuda.get_device_name(0)}",
             f"reps {args.reps} per timing ({max(1, args.reps // 4)} for the K-pass rows), median of {args.rounds} rounds"
             " [min .. max], ms per call, HIP events",
             f"36 candidates name the true rate of {n - wrong} / {n} streams; smallest runner_up - score = {gap};"
             f" chain payloads right on {decoded} / {min(n, 4096)} checked"]
    for name in variants:
        lines.append(f"  {name:32s} {med[name]:9.3f}  [{min(ms[name]):.3f} .. {max(ms[name]):.3f}]")
    lines.append("ratios (medians):")
    for k in ks:
        lb = lds_bytes(candidates_for(k), None) * n
        lines.append(f"  K = {k:2d}: detect / K uniform passes = {med[f'detect {k}'] / med[f'{k} x demod uniform']:.3f};"
                     f" detect / one mixed pass = {med[f'detect {k}'] / med['demod mixed']:.3f};"
                     f" LDS reads {lb / 1e9:.1f} GB -> {lb / (med[f'detect {k}'] * 1e-3) / 1e12:.1f} TB/s"
                     f" = {lb / (med[f'detect {k}'] * 1e-3) / LDS_PEAK:.2f} of ~75 TB/s (ds_read_b32, chip)")
    lines.append("measured: the kernel's time (the detect rows: one launch each) and its LDS-rate fraction (above).")
    lines.append("not measured: whether 256 threads per stream is the right shape at this size -- one shape is built.")
    text = "\n".join(lines)
    print(text)
    if args.txt:
        with open(args.txt, "a") as f:
            f.write(text + "\n\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"tool": "detect_bench", "streams": n, "ms": ms, "wrong": wrong, "min_gap": gap}, f)


if __name__ == "__main__":
    main()
