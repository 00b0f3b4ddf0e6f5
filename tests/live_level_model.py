"""The level tracker's rule (afskmodem_amd/csrc/afsk_live_level.hip) in numpy, and the gate of a
leveled live receiver driven by it: per channel a noise floor F, a decaying peak P and the threshold pair in force,
updated ahead of every push over the whole 2048-sample blocks the push walks (blocks from carry + chunk, a block that
meets the muted columns skipped, F and the pair frozen while a burst records), then the listen state machine of
``Receiver.__listen`` (ref:299-319) over the same blocks with the channel's pair.  tests/test_live_level_host.py pins the
update steps by hand, the gate against the CPU oracle's at fixed thresholds, and the issue's scenario table; the GPU
tests compare the device with it bit for bit.  Not a test module."""
from __future__ import annotations

import numpy as np

BLOCK = 2048
OPEN_END = 1
DEFAULTS = dict(start_q15=18000, end_q15=14000, floor_start_q8=512, floor_end_q8=384, min_start=1024, min_end=768,
                decay_shift=2, rise_shift=6)


def amplitude(block) -> int:
    """The gate's block amplitude: sum |x| >> 11 (ref:94-98 over 2048 samples)."""
    return int(np.abs(np.asarray(block, np.int64)).sum()) >> 11


def step(F: int, P: int, pp: int, A: int, rec: bool, p=DEFAULTS):
    """One block of amplitude A: the new (F, P, pp)."""
    P = A if A > P else P - ((P - A + (1 << p["decay_shift"]) - 1) >> p["decay_shift"])
    pp = max(pp, P)
    if not rec:
        F = A if F < 0 else (F - ((F - A + 3) >> 2) if A < F else F + ((A - F) >> p["rise_shift"]))
    return F, P, pp


def pair(F: int, pp: int, p=DEFAULTS):
    """The threshold pair after a walk that left floor F and saw the peak pp."""
    Fz = max(F, 0)
    start = min(65535, max((p["start_q15"] * pp) >> 15, (p["floor_start_q8"] * Fz) >> 8, p["min_start"]))
    end = min(65535, max((p["end_q15"] * pp) >> 15, (p["floor_end_q8"] * Fz) >> 8, p["min_end"]))
    return start, end


def clamp_mute(lo: int, hi: int, ln: int):
    lo = min(max(lo, 0), ln)
    return lo, min(max(hi, lo), ln)


class Channel:
    """One channel of a leveled receiver: LiveChan's pos / mode / rec_start / rec_len, the carry, the level row."""

    def __init__(self, start0: int, end0: int, params=DEFAULTS, leveled: bool = True):
        self.p, self.leveled = dict(params), leveled
        self.start0, self.end0 = start0, end0
        self.reset()

    def reset(self):
        self.row = [-1, 0, self.start0, self.end0]          # floor, peak, start, end
        self.new_stream()

    def new_stream(self):
        self.pos, self.mode, self.rec_start, self.blocks = 0, 0, 0, []
        self.carry = np.zeros(0, np.int16)

    @property
    def thresholds(self):
        return self.row[2], self.row[3]

    def track(self, x, mute=(0, 0)):
        """The tracker over the push of samples x (this channel's clamped length of them): the amplitudes it took."""
        x = np.asarray(x, np.int16)
        cl = self.pos & (BLOCK - 1)
        assert cl == self.carry.size
        lo, hi = clamp_mute(mute[0], mute[1], x.size)
        nblk = (cl + x.size) // BLOCK
        F, P = self.row[0], self.row[1]
        pp, rec, amps = P, self.mode == 2, []
        for b in range(nblk):
            col0 = b * BLOCK - cl
            if lo < hi and lo < col0 + BLOCK and hi > col0:
                continue                                     # a muted column: skipped, nothing updated
            blk = np.concatenate([self.carry, x[:BLOCK - cl]]) if b == 0 else x[col0:col0 + BLOCK]
            A = amplitude(blk)
            amps.append(A)
            F, P, pp = step(F, P, pp, A, rec, self.p)
        self.row[0], self.row[1] = F, P
        if not rec:
            self.row[2], self.row[3] = pair(F, pp, self.p)
        return amps

    def gate(self, x, flush: bool = False, mute=(0, 0)):
        """The push of samples x with the pair in force: the bursts it closes, as dicts (start, len, flags, the pair
        the burst opened with, its samples)."""
        x = np.asarray(x, np.int16).copy()
        lo, hi = clamp_mute(mute[0], mute[1], x.size)
        x[lo:hi] = 0
        cl = self.pos & (BLOCK - 1)
        s = np.concatenate([self.carry, x])
        nblk = s.size // BLOCK
        bpos0 = self.pos - cl
        out = []
        for b in range(nblk):
            blk = s[b * BLOCK:(b + 1) * BLOCK]
            amp = amplitude(blk)
            if self.mode == 0:
                self.mode = 1
                continue
            if self.mode == 1:
                if amp > self.row[2]:
                    self.mode, self.rec_start, self.blocks = 2, bpos0 + b * BLOCK, [blk]
                    self.open_pair = (self.row[2], self.row[3])
                continue
            self.blocks.append(blk)
            if amp < self.row[3]:
                out.append(self._burst(0))
                self.mode = 0
        if flush:
            if self.mode == 2:
                out.append(self._burst(OPEN_END))
            self.new_stream()
        else:
            self.carry = s[nblk * BLOCK:]
            self.pos += x.size
        return out

    def _burst(self, flags: int):
        samples = np.concatenate(self.blocks)
        return dict(start=self.rec_start, len=samples.size, flags=flags, amp_start=self.open_pair[0],
                    amp_end=self.open_pair[1], samples=samples)

    def push(self, x, flush: bool = False, mute=(0, 0), T: int | None = None):
        """Tracker, then gate.  T: the push's width (default len(x)); the tracker runs for every channel of a push with
        T > 0, also one whose own length is 0 (it walks no block and still derives the pair from the row)."""
        if self.leveled and (len(x) if T is None else T) > 0:
            self.track(x, mute)
        return self.gate(x, flush, mute)


class Receiver:
    """n channels; ``push`` takes what ``LiveReceiver.push`` takes (a [n, T] chunk, lengths, a flush bool or mask, mute
    ranges) and returns the closed bursts per channel."""

    def __init__(self, n: int, start0: int = 18000, end0: int = 14000, params=DEFAULTS, leveled: bool = True):
        self.ch = [Channel(start0, end0, params, leveled) for _ in range(n)]

    @property
    def state(self) -> np.ndarray:
        return np.asarray([c.row for c in self.ch], np.int32).reshape(-1, 4)

    def push(self, chunk, lengths=None, flush=False, mute=None):
        chunk = np.asarray(chunk, np.int16)
        T = chunk.shape[1]
        out = []
        for c, ch in enumerate(self.ch):
            ln = T if lengths is None else min(max(int(lengths[c]), 0), T)
            fl = bool(flush[c]) if np.ndim(flush) else bool(flush)
            m = (0, 0) if mute is None else (int(mute[c][0]), int(mute[c][1]))
            out.append(ch.push(chunk[c, :ln], fl, m, T))
        return out

    def reset(self, mask=None):
        for c, ch in enumerate(self.ch):
            if mask is None or mask[c]:
                ch.reset()
