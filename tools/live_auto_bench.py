#!/usr/bin/env python3
"""live_auto_bench.py -- the auto-rate streaming receiver's push (LiveReceiver(n, "auto"), afsk_live_push_auto) against
the fixed-rate streaming receiver's on the same buffers, in one process.

    python tools/live_auto_bench.py [--shapes 65536x2048,65536x8192] [--seconds 2] [--reps 3] [--parent PARENT.so]
                                    [--json OUT] [--txt OUT]

Per shape (channels x T samples per push): tools/live_bench.py's 1200-baud workload (two bursts per channel with
payloads of 4 / 12 / 24 bytes at random leads, every eighth channel silent, noise at 30 dB).  Every push is a column
window of that buffer, captured once into a graph per window position and replayed with device events around each
replay; the variants take turns pass by pass after one warm-up pass each (tools/live_bench.py's timed_pass), so drift
hits all alike:
  parent, parent_again   with --parent (a libafsk_amd.so of the parent commit): that build's fixed-rate streaming push,
                         twice -- the spread of the repeat is the margin this build's fixed-rate push has to stay inside
  fixed                  this build's fixed-rate streaming push at 1200 baud (the same kernel as the parent's)
  auto_1 / auto_4 / auto_36   the auto receiver with candidates [40], [20, 40, 80, 160] and all 36
Reported per variant: the mean us per push, its ratio to `fixed`, and the slowest window position (the mean over the
passes of the one push that took longest: where most bursts have their rate decided).  Then the WORST CASE: every
channel carries channel 1's samples, so every channel opens its burst in the same push -- the decision is K clock
searches on one wave per channel, all in one launch; the same variants, the slowest window position is the figure.
An eager pass of auto_36 counts the payloads decoded (against what was sent) and the rates named (1200 baud) out of
the bursts sent."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from afskmodem_amd import batch, synth  # noqa: E402
from afskmodem_amd.live import LiveReceiver  # noqa: E402
from live_bench import BAUD, BF, graphs_for, load_build, timed_pass, using  # noqa: E402

CANDIDATES = {"auto_1": [BF], "auto_4": [20, 40, 80, 160], "auto_36": list(batch.VALID_BIT_FRAMES)}


def timed_variants(torch, samples, n_push, T, reps, parent):
    """Every variant's per-window times over `reps` passes: {name: [reps, n_push] us}."""
    n = samples.shape[0]
    variants = ([("parent", parent, BF, {}), ("parent_again", parent, BF, {})] if parent is not None else []) \
        + [("fixed", None, BF, {})] + [(k, None, "auto", dict(candidates=c)) for k, c in CANDIDATES.items()]
    runs = []
    for name, lib, bf, kw in variants:
        with using(lib):
            rx = LiveReceiver(n, bf, max_burst_len=None, max_payload_len=256, max_chunk_len=T, **kw)
            out = rx.alloc_result()
            graphs = graphs_for(torch, rx, samples, n_push, T, out)
        runs.append(dict(name=name, lib=lib, rx=rx, graphs=graphs, out=out, passes=[]))
    for r in range(reps + 1):
        for v in runs:
            with using(v["lib"]):
                t = timed_pass(torch, v["rx"], v["graphs"])
            if r:
                v["passes"].append(t)
    torch.cuda.synchronize()
    times = {v["name"]: np.asarray(v["passes"]) for v in runs}
    for v in runs:
        del v["graphs"], v["out"]
        with using(v["lib"]):
            v["rx"].close()
    return times


def cells(times):
    out = {}
    for name, t in times.items():
        per_pass = t.mean(axis=1)
        per_window = t.mean(axis=0)
        out[name] = dict(us_mean=round(float(t.mean()), 2), us_passes=[round(float(x), 2) for x in per_pass],
                         spread=round(float((per_pass.max() - per_pass.min()) / per_pass.mean()), 4),
                         us_slowest_window=round(float(per_window.max()), 2), slowest_window=int(per_window.argmax()))
    for name, c in out.items():
        c["over_fixed"] = round(c["us_mean"] / out["fixed"]["us_mean"], 4)
        c["slowest_over_fixed_slowest"] = round(c["us_slowest_window"] / out["fixed"]["us_slowest_window"], 4)
    if "parent" in out:
        a, b = out["parent"]["us_mean"], out["parent_again"]["us_mean"]
        margin = max(abs(a - b) / min(a, b), out["parent"]["spread"], out["parent_again"]["spread"])
        out["margin"] = round(margin, 4)
        out["fixed_over_parent"] = round(out["fixed"]["us_mean"] / (0.5 * (a + b)), 4)
        out["fixed_inside_margin"] = bool(out["fixed"]["us_mean"] <= max(a, b) * (1 + margin))
    return out


def decoded_and_named(torch, samples, sent, n_push, T):
    """An eager pass of the auto receiver with all 36 candidates: (payloads decoded, rates named, bursts sent)."""
    n = samples.shape[0]
    rx = LiveReceiver(n, "auto", max_burst_len=None, max_payload_len=256, max_chunk_len=T)
    out, ev = rx.alloc_result(), rx.alloc_events()
    got = [[] for _ in range(n)]
    for p in range(n_push):
        # (the packed event list: the host copies the closed bursts' records, payloads and rates, not every slot)
        res = rx.push(samples[:, p * T: (p + 1) * T], out=out, flush=p == n_push - 1, events=ev)
        for (c, _, _, payload), bf in zip(res.events.bursts(), res.events.bit_frames().tolist()):
            got[c].append((payload, bf))
    rx.close()
    total = sum(len(s) for s in sent)
    decoded = named = 0
    for c in range(n):
        want = [b for _, b in sent[c]]
        for (payload, bf), w in zip(got[c], want):
            decoded += payload == w
            named += bf == BF
    return decoded, named, total


def run_shape(torch, n, T, seconds, reps, seed, parent):
    total = int(seconds * 48000)
    n_push = total // T
    total = n_push * T
    samples, sent = synth.live_channels(n, total, BAUD, seed, bursts_per_channel=2, payload_lens=(4, 12, 24),
                                        silent_every=8, device="cuda")
    decoded, named, bursts = decoded_and_named(torch, samples, sent, n_push, T)
    rec = dict(shape=f"{n}x{T}", baud=BAUD, pushes=n_push, reps=reps, bursts_sent=bursts, payloads_decoded=decoded,
               rates_named=named, workload=cells(timed_variants(torch, samples, n_push, T, reps, parent)))
    samples[:] = samples[1].clone()                         # the worst case: every channel opens in the same push
    torch.cuda.synchronize()
    rec["worst_case"] = cells(timed_variants(torch, samples, n_push, T, reps, None))
    del samples
    torch.cuda.empty_cache()
    return rec


def lines_of(rec):
    out = [f"{rec['shape']} @{rec['baud']}  {rec['pushes']} pushes per pass, {rec['reps']} passes; auto_36 (eager): "
           f"payloads decoded {rec['payloads_decoded']}/{rec['bursts_sent']}, rates named "
           f"{rec['rates_named']}/{rec['bursts_sent']}"]
    for part in ("workload", "worst_case"):
        c = rec[part]
        out.append(f"  {part}: us per push, mean (x fixed) | slowest window position (x fixed's slowest)")
        for name in ("parent", "parent_again", "fixed", "auto_1", "auto_4", "auto_36"):
            if name in c:
                v = c[name]
                out.append(f"    {name:13s} {v['us_mean']:10.1f} x{v['over_fixed']:.4f} (spread {100 * v['spread']:.2f} %) | "
                           f"{v['us_slowest_window']:10.1f} x{v['slowest_over_fixed_slowest']:.4f} (window "
                           f"{v['slowest_window']})")
        if "margin" in c:
            out.append(f"    fixed/parent x{c['fixed_over_parent']:.4f} (margin {100 * c['margin']:.2f} %: "
                       f"{'inside' if c['fixed_inside_margin'] else 'OUTSIDE'})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x2048,65536x8192")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--parent", help="libafsk_amd.so of the parent commit: its fixed-rate streaming push, timed in the same run")
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    import torch
    parent = load_build(args.parent) if args.parent else None
    res, lines = [], []
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        rec = run_shape(torch, n, T, args.seconds, args.reps, args.seed, parent)
        print(json.dumps(rec), flush=True)
        res.append(rec)
        lines += lines_of(rec)
    print("\n".join(lines))
    for path, text in ((args.json, json.dumps(dict(tool="tools/live_auto_bench.py", parent=bool(args.parent),
                                                   seconds=args.seconds, reps=args.reps, results=res), indent=1)),
                       (args.txt, "\n".join(lines) + "\n")):
        if path:
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
