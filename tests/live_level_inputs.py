"""Seeded inputs of the level tracker's tests (tests/test_gpu_live_level.py, and tests/test_live_level_host.py for the
conditions the GPU tests rest on): the parity streams, the one-burst-per-channel captures and the push plan that mixes
plain, ragged, muted and flushing pushes.  Not a test module."""
import numpy as np

import afskmodem_amd as afskmodem

BLOCK = 2048
N = 70                                                   # channels: not a multiple of the four waves of a block
GAINS = (1.0, 0.5, 0.25, 0.125, 0.0625)
SIGMAS = (300.0, 1500.0, 3000.0)
TRAINING = 0.2
PARITY_LEN = 61 * BLOCK                                  # 2.6 s
PAIR_LEN = 23 * 4096                                     # 1.96 s
PAIR_T = 4096


def message(bf: int, payload: bytes) -> np.ndarray:
    return afskmodem.Transmitter(48000 // bf, TRAINING).wav_samples(payload).astype(np.float64)


def payload_of(c: int, k: int = 0) -> bytes:
    return b"ch%03d msg%d ok" % (c, k)


def finish(rng, x, sigma: float, total: int) -> np.ndarray:
    x = np.concatenate([x, np.zeros(max(total - x.size, 0))])[:total]
    return np.clip(np.rint(x + rng.normal(0, sigma, total)), -32768, 32767).astype(np.int16)


def parity_streams(seed: int = 5) -> np.ndarray:
    """[N, PARITY_LEN]: two transmissions (gains 1 ... 1/16) over noise of three sigmas at odd offsets, noise alone,
    zeros and both rails."""
    rng = np.random.default_rng(seed)
    specs = [("tx", g, s) for s in SIGMAS for g in range(len(GAINS))] * 4
    specs += [("noise", 0, s) for s in SIGMAS] + [("zeros", 0, 0.0), ("rail", 32767, 0.0), ("rail", -32768, 0.0)]
    specs += specs[:N - len(specs)]
    rows = []
    for c, (kind, g, sigma) in enumerate(specs[:N]):
        if kind == "tx":
            w = message(40, payload_of(c))
            lead = int(0.8 * 48000) + int(rng.integers(0, BLOCK))
            gap = int(0.6 * 48000) + int(rng.integers(0, BLOCK))
            x = np.concatenate([np.zeros(lead), w * GAINS[g], np.zeros(gap), w * GAINS[(g + 2 + c // 15) % len(GAINS)]])
            rows.append(finish(rng, x, sigma, PARITY_LEN))
        elif kind == "noise":
            rows.append(finish(rng, np.zeros(0), sigma, PARITY_LEN))
        elif kind == "zeros":
            rows.append(np.zeros(PARITY_LEN, np.int16))
        else:
            rows.append(np.full(PARITY_LEN, g, np.int16))
    return np.stack(rows)


def pair_rates(kind: str) -> np.ndarray:
    """The channels' bit_frames of a receiver kind: "fixed" and "progressive" 1200 baud, "mixed" and "auto" 1200 and 600
    baud alternating."""
    return np.asarray([40 if kind in ("fixed", "progressive") or c % 2 == 0 else 80 for c in range(N)], np.int32)


def pair_streams(rates, seed: int = 9):
    """([N, PAIR_LEN], payloads): one burst per channel behind a noise lead-in of at least 0.9 s, gains 1 ... 1/8 over
    sigma 300, 1000 or 2000; every seventh channel is noise alone."""
    rng = np.random.default_rng(seed)
    rows, sent = [], []
    for c in range(N):
        sigma = (300.0, 1000.0, 2000.0)[c % 3]
        if c % 7 == 6:
            rows.append(finish(rng, np.zeros(0), sigma, PAIR_LEN))
            sent.append(None)
            continue
        lead = int(0.9 * 48000) + int(rng.integers(0, BLOCK))
        x = np.concatenate([np.zeros(lead), message(int(rates[c]), payload_of(c)) * GAINS[(c // 3) % 4]])
        assert x.size + 4 * BLOCK <= PAIR_LEN
        rows.append(finish(rng, x, sigma, PAIR_LEN))
        sent.append(payload_of(c))
    return np.stack(rows), sent


def push_plan(T: int, total: int, seed: int = 3):
    """The pushes of the parity test over streams of ``total`` samples: dicts with ``lens`` ([N] or None: plain),
    ``mute`` ([N, 2] or None), ``flush`` ([N] bool or None), ``reset`` ([N] bool or None: reset(mask) ahead of the
    push), and the stream columns ``cur`` every channel's row starts at.  Lengths include 0 and T; mute ranges miss the
    push, cut a block, cover whole blocks and lie outside 0 ... T (clamped)."""
    rng = np.random.default_rng(seed + T)
    cur = np.zeros(N, np.int64)
    n_push = -(-total // T)
    plan = []
    for i in range(n_push):
        left = total - cur
        kind = i % 5
        lens = mute = flush = reset = None
        if kind in (1, 3):
            pick = rng.integers(0, 4, N)
            lens = np.where(pick == 0, 0, np.where(pick == 1, T, rng.integers(1, T + 1, N)))
        if kind in (2, 3):
            pick = rng.integers(0, 5, N)
            lo = rng.integers(0, T, N)
            mute = np.stack([lo, lo + rng.integers(1, BLOCK, N)], axis=1)          # cuts one or two blocks
            mute[pick == 0] = (5, 5)                                                # misses
            mute[pick == 1] = (-7, T + 9)                                           # covers the push (clamped)
            mute[pick == 2, 1] = mute[pick == 2, 0] + 2 * BLOCK + 17                # covers a whole block where T allows
            mute[pick == 3] = (T, 2 * T)                                            # beyond the push: misses
        if kind == 3 and i > 2:
            flush = rng.integers(0, 5, N) == 0
        if i == n_push // 2:
            reset = rng.integers(0, 3, N) == 0
        if lens is None and (left < T).any():
            lens = np.full(N, T)
        if lens is not None:
            lens = np.minimum(lens, left).astype(np.int32)
        plan.append(dict(cur=cur.copy(), lens=lens, mute=None if mute is None else mute.astype(np.int32), flush=flush,
                         reset=reset))
        cur = cur + (T if lens is None else lens)
    return plan


def chunk_of(streams, step, T: int) -> np.ndarray:
    """The [N, T] chunk of a plan step: channel c's row holds its stream from cur[c] on, for the channel's length; the
    columns at and beyond the length hold full scale, so a read beyond a length would show."""
    out = np.full((N, T), 32767, np.int16)
    for c in range(N):
        ln = T if step["lens"] is None else int(step["lens"][c])
        out[c, :ln] = streams[c, step["cur"][c]: step["cur"][c] + ln]
    return out
