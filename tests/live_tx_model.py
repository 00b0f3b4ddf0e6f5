"""A pure-Python model of the live transmitter's queues (afsk_live_tx_*, ``LiveTransmitter``): statuses, starts,
retirement, reset, and the expected samples of a pull.  tests/test_live_tx_host.py pins it against hand-worked cases;
tests/test_gpu_live_tx.py uses it as the expected value.  Not a test module."""
from __future__ import annotations

from collections import deque

import numpy as np

from afskmodem_amd import _native

TAIL = 4800


class LiveTxModel:
    def __init__(self, n_channels: int, bit_frames: int, ts_cycles: int, queue_depth: int, max_payload_len: int,
                 wav=None):
        self.n, self.bf, self.ts = n_channels, bit_frames, max(ts_cycles, 0)
        self.depth, self.max_payload = queue_depth, max_payload_len
        self.wav = wav                                      # payload bytes -> .wav samples (only for expected())
        self.pos = [0] * n_channels
        self.end = [0] * n_channels
        self.queue = [deque() for _ in range(n_channels)]   # (start, n_samples) not yet fully emitted
        self.on_air = [[] for _ in range(n_channels)]       # (start, n_samples, payload) not yet fully pulled

    def n_samples(self, plen: int) -> int:
        return self.bf * (2 * self.ts + 4 + 14 * plen) + TAIL

    def submit(self, channels, payloads, sort: bool = True):
        """(status, start, n_samples) per message in the caller's order.  sort=True: the Python layer's stable sort
        (bad channels first); sort=False: the C entry's rule -- from the first message whose channel is below its
        predecessor's on, AFSK_LIVE_TX_UNSORTED."""
        payloads = [p.encode() if isinstance(p, str) else bytes(p) for p in payloads]
        ch = [int(c) for c in channels]
        m = len(payloads)
        status, start, ns = [0] * m, [-1] * m, [0] * m
        if sort:
            order = sorted(range(m), key=lambda i: ch[i] if 0 <= ch[i] < self.n else -1)
            first_bad = m
        else:
            order = list(range(m))
            first_bad = next((i for i in range(1, m) if ch[i] < ch[i - 1]), m)
        for k, i in enumerate(order):
            c, p = ch[i], payloads[i]
            if k >= first_bad:
                status[i] = _native.LIVE_TX_UNSORTED
            elif not 0 <= c < self.n:
                status[i] = _native.LIVE_TX_BAD_CHANNEL
            elif len(p) > self.max_payload:
                status[i] = _native.LIVE_TX_TOO_LONG
            elif len(self.queue[c]) >= self.depth:
                status[i] = _native.LIVE_TX_QUEUE_FULL
            else:
                s, n = max(self.pos[c], self.end[c]), self.n_samples(len(p))
                self.queue[c].append((s, n))
                self.on_air[c].append((s, n, p))
                self.end[c] = s + n
                status[i], start[i], ns[i] = _native.LIVE_TX_QUEUED, s, n
        return np.array(status, np.int32), np.array(start, np.int64), np.array(ns, np.int32)

    def expected(self, T: int) -> np.ndarray:
        """int16 [n, T]: samples [pos, pos + T) of every channel (does not advance)."""
        out = np.zeros((self.n, T), np.int16)
        for c in range(self.n):
            lo, hi = self.pos[c], self.pos[c] + T
            for s, n, p in self.on_air[c]:
                a, b = max(s, lo), min(s + n, hi)
                if a < b:
                    out[c, a - lo: b - lo] = self.wav(p)[a - s: b - s]
        return out

    def pull(self, T: int) -> np.ndarray:
        """Advance every channel by T, retire what ended; returns pending (int32 [n])."""
        for c in range(self.n):
            self.pos[c] += T
            q = self.queue[c]
            while q and q[0][0] + q[0][1] <= self.pos[c]:
                q.popleft()
            self.on_air[c] = [e for e in self.on_air[c] if e[0] + e[1] > self.pos[c]]
        return self.pending()

    def pending(self) -> np.ndarray:
        return np.array([len(q) for q in self.queue], np.int32)

    def reset(self, mask=None) -> None:
        for c in range(self.n):
            if mask is None or mask[c]:
                self.pos[c] = self.end[c] = 0
                self.queue[c].clear()
                self.on_air[c] = []
