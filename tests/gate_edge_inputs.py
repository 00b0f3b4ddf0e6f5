"""Inputs of tests/test_gpu_gate_edges.py (not a test module): captures whose 2048-sample block amplitudes sit exactly
on a gate threshold, and what the CPU oracle's whole-capture gate (``O.gate_stream``, Receiver.__listen ref:299-319)
reports for them.  A square wave +a, -a, ... has getAmplitude == a exactly (ref:94-98).

  sequences / live_rows / flat_captures   every six-block sequence over five class amplitudes of a threshold pair
  every_sample_rows                        [silence, X_p, silence] for p = 0 ... 2047, where sample p alone decides
                                           whether the block reaches 18001
  expected_events                          the oracle's bursts of every row as one (channel, start, len, flags) table"""
import functools
import itertools

import numpy as np

from afskmodem_amd import _native
from oracle import afsk_oracle as O

BLOCK = 2048
N_BLOCKS = 6
N_SEQ = 5 ** N_BLOCKS
PAIRS = ((18000, 14000), (14000, 18000), (16000, 16000))


def class_amps(pair):
    """The five block amplitudes around a pair: silence, one below / on amp_end, on / one above amp_start; for an
    equal pair one below / on / one above it and a loud one."""
    s, e = pair
    return (0, e - 1, e, s, s + 1) if s != e else (0, s - 1, s, s + 1, 30000)


@functools.lru_cache(maxsize=None)
def sequences() -> np.ndarray:
    """int64 [15625, 6]: every sequence of six class indices."""
    return np.array(list(itertools.product(range(5), repeat=N_BLOCKS)), np.int64)


def square_rows(amps) -> np.ndarray:
    """int16 [n, k * 2048] from int [n, k] block amplitudes."""
    amps = np.asarray(amps, np.int16)
    sign = np.tile(np.array([1, -1], np.int16), BLOCK // 2)
    return (amps[:, :, None] * sign[None, None, :]).reshape(amps.shape[0], amps.shape[1] * BLOCK)


@functools.lru_cache(maxsize=1)
def live_rows(pair) -> np.ndarray:
    """int16 [15625, 12288]: row i holds the six exact blocks of sequence i over the pair's class amplitudes."""
    return square_rows(np.array(class_amps(pair), np.int64)[sequences()])


def flat_captures(pair, seed=3):
    """The 15625 captures back to back as gate_batch takes them: every third one with a random tail of 1 ... 2047
    samples (a partial block the gate must ignore), gaps of 0 ... 2 loud samples between them (odd and even
    offsets).  -> (flat int16, stream_offset int64 [n], stream_len int32 [n])."""
    rows = live_rows(pair)
    rng = np.random.default_rng(seed)
    n, base = rows.shape
    tail = np.where(np.arange(n) % 3 == 0, rng.integers(1, BLOCK, n), 0)
    gap = rng.integers(0, 3, n)
    ln = (base + tail).astype(np.int32)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum(ln[:-1].astype(np.int64) + gap[:-1])
    flat = np.full(int(off[-1]) + int(ln[-1]) + 2, 32767, np.int16)
    noise = rng.integers(-32768, 32768, int(tail.sum())).astype(np.int16)
    used = 0
    for i in range(n):
        o = int(off[i])
        flat[o: o + base] = rows[i]
        if tail[i]:
            flat[o + base: o + base + tail[i]] = noise[used: used + tail[i]]
            used += int(tail[i])
    return flat, off, ln


def expected_gate(flat, off, ln, pair, max_bursts):
    """O.gate_stream of every capture -> n_bursts [n], burst_start / burst_len [n, max_bursts] (0 past n_bursts),
    open_end [n]."""
    n = len(off)
    nb, oe = np.zeros(n, np.int32), np.zeros(n, np.int32)
    bs, bl = np.zeros((n, max_bursts), np.int32), np.zeros((n, max_bursts), np.int32)
    for i in range(n):
        bursts, oe[i] = O.gate_stream(flat[off[i]: off[i] + ln[i]], pair[0], pair[1], max_bursts)
        nb[i] = len(bursts)
        for k, (s, m) in enumerate(bursts):
            bs[i, k], bl[i, k] = s, m
    return nb, bs, bl, oe


def expected_events(rows, amp_start, amp_end) -> np.ndarray:
    """int64 [m, 4]: (channel, start, len, flags) of every burst O.gate_stream(rows[c], ..., 64) reports, channel by
    channel in time order, LIVE_OPEN_END on a burst still open at the end of the row (what a flush reports).
    amp_start / amp_end: one value or one per row."""
    n = len(rows)
    starts, ends = np.broadcast_to(amp_start, (n,)), np.broadcast_to(amp_end, (n,))
    out = []
    for c in range(n):
        bursts, oe = O.gate_stream(rows[c], int(starts[c]), int(ends[c]), 64)
        for k, (s, m) in enumerate(bursts):
            out.append((c, s, m, _native.LIVE_OPEN_END if oe and k == len(bursts) - 1 else 0))
    return np.array(out, np.int64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def expected_live(pair) -> np.ndarray:
    return expected_events(live_rows(pair), *pair)


@functools.lru_cache(maxsize=1)
def every_sample_rows() -> np.ndarray:
    """int16 [4096, 6144], rows [silence, X, silence].  Row p < 2048: X is +-18000 with |x[p]| raised by 2048, so
    sum |x| = 2048 * 18001 and the amplitude is exactly 18001 -- the burst opens at (18000, 14000) only if sample p
    reached the sum.  Row 2048 + p: +-18001 with |x[p]| lowered by 1, amplitude 18000 -- it must not open, and would
    if sample p were left out in favour of a neighbour or counted by its neighbour's value."""
    rows = square_rows(np.array([[0, 18000, 0]] * BLOCK + [[0, 18001, 0]] * BLOCK)).astype(np.int32)
    p = np.arange(BLOCK)
    sign = np.where(p % 2 == 0, 1, -1)
    rows[p, BLOCK + p] += 2048 * sign
    rows[BLOCK + p, BLOCK + p] -= sign
    return rows.astype(np.int16)
