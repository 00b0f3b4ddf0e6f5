"""Shared by the GPU tests of the live receivers and transmitters (tests/test_gpu_live*.py): a push's bursts as rows of
dicts, push sizes, the driver that pushes a capture into one result and flushes, and the seeded captures and payloads.
Not a test module.  A test whose call pattern or compared fields differ keeps a helper of its own, under its own name."""
import numpy as np

import afskmodem_amd as afskmodem

BLOCK = 2048
FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")


def collect(res, got, corrected=False):
    """Append one push's bursts to got[c] as dicts (synchronises): start, len, flags, every demod field, the row up to
    nbytes; ``corrected`` when asked for, and the rate outputs of an auto receiver's push."""
    nc = res.n_closed.cpu().numpy()
    if not nc.any():
        return
    bs, bl, fl = (t.cpu().numpy() for t in (res.burst_start, res.burst_len, res.flags))
    d = res.demod.cpu()
    cor = res.demod.corrected.cpu().numpy() if corrected else None
    rate = None if res.bit_frames is None else (res.bit_frames.cpu().numpy(), res.rate_score.cpu().numpy())
    s = res.slots
    for c in np.nonzero(nc)[0].tolist():
        for k in range(int(nc[c])):
            j = c * s + k
            row = dict(start=int(bs[c, k]), len=int(bl[c, k]), flags=int(fl[c, k]),
                       bytes=d.bytes[j, : min(int(d.nbytes[j]), d.bytes.shape[1])].tobytes())
            row.update({f: int(getattr(d, f)[j]) for f in FIELDS})
            if corrected:
                row["corrected"] = int(cor[j])
            if rate:
                row["bit_frames"], row["rate_score"] = int(rate[0][c, k]), int(rate[1][c, k])
            got[c].append(row)


def push_sizes(kind, total, rng=None, steps=None):
    """Push sizes summing to total: "whole", a fixed step (an int or its decimal string; [0] for no samples at all), or
    -- "ragged", "random" -- one ``rng.choice(steps)`` per push.  The seeded draws decide which inputs a test sees, so
    every caller passes the step set it always drew from."""
    if kind == "whole":
        return [total]
    if kind in ("ragged", "random"):
        out, left = [], total
        while left > 0:
            t = min(int(rng.choice(steps)), left)
            out.append(t)
            left -= t
        return out
    step = int(kind)
    return [min(step, total - p) for p in range(0, total, step)] or [0]


def drive(rx, d, sizes, corrected=False, flush=True, each=None):
    """Push the column windows of d ([n, L] device) of the given sizes into ONE result, then flush on its own;
    ``each(out)`` after every call.  The bursts per channel, as ``collect`` rows."""
    got = [[] for _ in range(rx.n_channels)]
    out = rx.alloc_result(diagnostics=corrected)
    p = 0
    for t in sizes:
        collect(rx.push(d[:, p: p + t], out=out), got, corrected)
        if each:
            each(out)
        p += t
    assert p == d.shape[1]
    if flush:
        collect(rx.flush(out=out), got, corrected)
        if each:
            each(out)
    return got


def same(got, want):
    """One channel's bursts against expected rows (every field the expected rows have)."""
    return len(got) == len(want) and all({k: g[k] for k in w} == w for g, w in zip(got, want))


def noisy(rng, x, sigma):
    return np.clip(x + rng.normal(0, sigma, x.size), -32768, 32767).astype(np.int16)


def capture_of(rng, bf, payloads, gap=3 * BLOCK, sigma=2000.0, training=0.5):
    """Messages with quiet gaps, in noise.  A message starts a random number of samples into a block, fewer than
    the clock search covers (4096 - 2 bf offsets) from 1000 samples per symbol on: the gate cuts bursts at block
    boundaries, so a slower message starting later in its block is not decodable, by the reference either."""
    tr = afskmodem.Transmitter(48000 // bf, training)
    lim = BLOCK if 4096 - 2 * bf >= BLOCK else 4096 - 2 * bf - 8
    parts, n = [], 0
    for p in payloads:
        pad = (-n) % BLOCK + gap + int(rng.integers(0, lim))
        parts += [np.zeros(pad, np.int16), tr.wav_samples(p)]
        n += pad + parts[-1].size
    parts.append(np.zeros(gap + int(rng.integers(0, BLOCK)), np.int16))
    return noisy(rng, np.concatenate(parts), sigma)


def random_payload(rng, lo, hi):
    """A payload of lo ... hi random bytes."""
    return bytes(rng.integers(0, 256, int(rng.integers(lo, hi + 1)), dtype=np.uint8))
