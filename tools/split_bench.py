#!/usr/bin/env python3
"""split_bench.py -- the few-long-streams shapes through today's entries and through the sequence-parallel path.

    python tools/split_bench.py [--reps 20] [--json OUT]

For every shape (1200 baud, clean signal): 1 x 600 s, 8 / 64 / 256 x 60 s, 2048 x 8 s, 16384 x 4 s, the ragged
0.25 ... 4 s batch, and config #5 (65536 x 1 s, for information) it times
  * the existing entry: demod_batch (the uniform kernel; a ragged batch goes through its length-sorted plan),
  * the split entry: demod_batch_split with a SplitPlan built once,
as the median ms per launch over --reps launches (HIP events around each launch, after two warm-up launches), and
prints the fraction of the 8 TB/s HBM peak using the algorithmic byte count 2 * (L - 4800 + bf) per stream (what a
decoder must read: everything but the tail silence).  Both results are checked against each other's payloads,
the round trip to the modulated payload, and the CPU oracle on up to 8 streams.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from afskmodem_amd import batch, synth  # noqa: E402

PEAK = 8.0e12
BAUD, BF = 1200, 40


def modulate(torch, lens, seed):
    n = len(lens)
    lens = np.asarray(lens, np.int32)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    plen = np.array([max(synth.one_second_payload(BAUD, 0.5, int(L)), 0) for L in lens], np.int32)
    stride = max(int(plen.max()), 1)
    payload = synth.payload_bytes(seed, 0, n, stride)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    samples = torch.empty(int(lens.sum()), dtype=torch.int16, device="cuda")
    batch.modulate_batch(t(payload), t(plen), t(np.full(n, BF, np.int32)),
                         t(np.full(n, synth.ts_cycles_for(BAUD), np.int32)), t(off), t(lens), int(lens.max()),
                         samples, False)
    torch.cuda.synchronize()
    return samples, t(off), t(lens), off, lens, payload, plen


def time_launches(torch, fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def run_shape(torch, name, lens, reps, seed, oracle):
    samples, d_off, d_ln, off, lens, payload, plen = modulate(torch, lens, seed)
    n = len(lens)
    stride = batch.out_stride_for(int(lens.max()), BF)
    algo = float(np.sum(2 * (lens.astype(np.int64) - 4800 + BF)))
    out_a = batch.alloc_result(n, stride, samples.device)
    out_b = batch.alloc_result(n, stride, samples.device)
    ragged = batch.lengths_ragged(lens)
    plan = batch.SplitPlan(lens, BF)
    fa = lambda: batch.demod_batch(samples, d_off, d_ln, BF, out=out_a,  # noqa: E731
                                   stream_len_host=lens if ragged else None)
    fb = lambda: batch.demod_batch_split(samples, d_off, d_ln, plan, out=out_b)  # noqa: E731
    ms_a = time_launches(torch, fa, reps)
    ms_b = time_launches(torch, fb, reps)
    ha, hb = out_a.cpu(), out_b.cpu()
    pa, pb = ha.payloads(), hb.payloads()
    same = all(np.array_equal(getattr(ha, f), getattr(hb, f)) for f in ("nbytes", "nbits", "clock_idx",
                                                                         "term_frame", "status")) and pa == pb
    roundtrip = all(pb[s] == payload[s, : plen[s]].tobytes() for s in range(n))
    oracle_ok = None
    if oracle is not None:
        pick = np.unique(np.linspace(0, n - 1, min(n, 8)).astype(np.int64))
        flat = samples.cpu().numpy()
        xs = [flat[off[s]: off[s] + lens[s]] for s in pick]
        o_off = np.zeros(len(pick), np.int64)
        o_off[1:] = np.cumsum([len(x) for x in xs[:-1]])
        want = oracle.demod_batch(np.concatenate(xs), o_off, lens[pick], np.full(len(pick), BF, np.int32), 14000,
                                  out_stride=stride, n_threads=8)
        oracle_ok = all(int(want["nbytes"][j]) == int(hb.nbytes[s]) and int(want["clock_idx"][j]) == int(hb.clock_idx[s])
                        and int(want["term_frame"][j]) == int(hb.term_frame[s]) and int(want["nbits"][j]) == int(hb.nbits[s])
                        and bytes(want["bytes"][j][: min(int(want["nbytes"][j]), stride)]) == pb[s][:stride]
                        for j, s in enumerate(pick))
    row = dict(shape=name, streams=n, samples=int(lens.sum()), segments=plan.n_segments,
               existing_ms=round(ms_a, 4), existing_frac=round(algo / (ms_a * 1e-3) / PEAK, 4),
               split_ms=round(ms_b, 4), split_frac=round(algo / (ms_b * 1e-3) / PEAK, 4),
               speedup=round(ms_a / ms_b, 2), same_outputs=bool(same), roundtrip=bool(roundtrip), oracle=oracle_ok)
    plan.close()
    del samples, out_a, out_b
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import torch
    oracle = None
    if not args.no_oracle:
        from oracle import afsk_oracle as oracle
    rng = np.random.default_rng(8)
    shapes = [
        ("1 x 600 s", [600 * 48000]),
        ("8 x 60 s", [60 * 48000] * 8),
        ("64 x 60 s", [60 * 48000] * 64),
        ("256 x 60 s", [60 * 48000] * 256),
        ("2048 x 8 s", [8 * 48000] * 2048),
        ("16384 x 4 s", [4 * 48000] * 16384),
        ("ragged 0.25 ... 4 s (16384)", list((rng.uniform(0.25, 4.0, 16384) * 48000).astype(np.int64))),
        ("config #5: 65536 x 1 s (information)", [48000] * 65536),
    ]
    rows = []
    for k, (name, lens) in enumerate(shapes):
        row = run_shape(torch, name, lens, args.reps, 100 + k, oracle)
        rows.append(row)
        print(f"{name:40s} existing {row['existing_ms']:9.4f} ms ({row['existing_frac']:.3f} of peak)   "
              f"split {row['split_ms']:9.4f} ms ({row['split_frac']:.3f})   x{row['speedup']:<6} "
              f"segments {row['segments']:7d}  same {row['same_outputs']}  roundtrip {row['roundtrip']}  "
              f"oracle {row['oracle']}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(peak_bytes_per_s=PEAK, baud=BAUD, rows=rows), f, indent=1)
    return 0 if all(r["same_outputs"] and r["roundtrip"] and r["oracle"] is not False for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
