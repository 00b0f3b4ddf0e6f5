"""A pure-Python model of carrier sense on the live side (afsk_live_busy, afsk_live_tx_pull_hold,
``LiveReceiver.busy``, ``LiveTransmitter.pull(hold=)``), written from the header's rules alone:

* ``HoldTxModel`` / ``HoldTxRatedModel``: the five-step hold rule on top of the queue models ``LiveTxModel`` and
  ``LiveTxRatedModel`` (imported, not edited) -- the wait counter ``w`` per channel, the shift of the messages that have
  not begun, ``deferred``, and the expected samples of a hold pull.
* ``BusyModel``: the reference's ``__listen`` gate (afskmodem.py:299-319) walked in 2048-sample blocks, one channel,
  fed push by push: ``busy`` is true while the gate is between "Recording started" and "Recording finished".

tests/test_live_tx_hold_host.py pins both against hand-worked cases and the bursts recorded in tests/golden/;
tests/test_gpu_live_hold.py uses them as the expected value.  They never see a kernel's output.  Not a test module."""
from __future__ import annotations

import numpy as np

from tests.live_tx_model import LiveTxModel
from tests.live_tx_rated_model import LiveTxRatedModel

BLOCK = 2048


class _HoldRule:
    """The hold rule over a queue model's ``pos``, ``end``, ``queue`` (start, n) and ``on_air`` (start, n, payload)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.wait = [0] * self.n                            # w: 0 after create

    def pull_hold(self, T: int, lens=None, hold=None, holdoff: int = 0, fill: int = 0):
        """One hold pull of T columns into a buffer that held ``fill``: ``(samples int16 [n, T], pending int32 [n],
        deferred int64 [n])``.  ``lens`` None: every channel advances T; ``hold`` None: nobody is held."""
        wait = self.wait
        L = [T if lens is None else min(max(int(lens[c]), 0), T) for c in range(self.n)]
        held = [bool(hold[c]) if hold is not None else False for c in range(self.n)]
        deferred = np.zeros(self.n, np.int64)
        for c in range(self.n):
            pos = self.pos[c]
            earliest = pos + L[c] if held[c] else pos + wait[c]                      # step 1
            q = list(self.queue[c])
            u = next((i for i, (s, _) in enumerate(q) if s >= pos), None)            # step 2
            if u is not None and q[u][0] < earliest:                                 # step 3
                delta = earliest - q[u][0]
                moved = {s for s, _ in q[u:]}
                self.queue[c].clear()
                self.queue[c].extend((s + delta, n) if i >= u else (s, n) for i, (s, n) in enumerate(q))
                self.on_air[c] = [(s + delta, n, p) if s in moved else (s, n, p) for s, n, p in self.on_air[c]]
                self.end[c] += delta
                deferred[c] = delta
        out = self.expected(T) if T else np.zeros((self.n, 0), np.int16)             # step 4: render ...
        for c in range(self.n):
            out[c, L[c]:] = fill
        for c in range(self.n):                                                      # ... and commit
            self.pos[c] += L[c]
            q = self.queue[c]
            while q and q[0][0] + q[0][1] <= self.pos[c]:
                q.popleft()
            self.on_air[c] = [e for e in self.on_air[c] if e[0] + e[1] > self.pos[c]]
            wait[c] = int(holdoff) if held[c] else max(0, wait[c] - L[c])            # step 5
        return out, self.pending(), deferred

    def reset(self, mask=None) -> None:
        super().reset(mask)
        for c in range(self.n):
            if mask is None or mask[c]:
                self.wait[c] = 0


class HoldTxModel(_HoldRule, LiveTxModel):
    """``LiveTxModel`` (one geometry) with ``pull_hold``."""


class HoldTxRatedModel(_HoldRule, LiveTxRatedModel):
    """``LiveTxRatedModel`` (a geometry per message out of a table) with ``pull_hold``.  A one-entry table is the
    uniform transmitter, a message of channel c at entry ``entry_of_channel[c]`` the mixed one."""


class BusyModel:
    """One channel of ``Receiver.__listen`` fed push by push.  The reference reads 2048-sample blocks: it discards the
    first (ref:303), waits for a block whose amplitude is above ``amp_start`` (ref:306: "Recording started"), then
    records every block up to and including the first whose amplitude is below ``amp_end`` (ref:314-318: "Recording
    finished") and starts over -- the next call of ``__listen`` discards a block again.  ``busy`` is true exactly
    while the gate records.  ``Waveforms.getAmplitude`` is the mean of the absolute values, floored (sum >> 11)."""

    def __init__(self, amp_start: int = 18000, amp_end: int = 14000):
        self.amp_start, self.amp_end = int(amp_start), int(amp_end)
        self.reset()

    def reset(self) -> None:
        self.mode = 0                                       # 0: discard a block, 1: wait for a start, 2: recording
        self.carry = np.zeros(0, np.int16)                  # the partial block at the end of the stream
        self.pos = 0

    @property
    def busy(self) -> int:
        return int(self.mode == 2)

    def push(self, samples, flush: bool = False) -> int:
        """Append ``samples`` and walk every whole block; ``flush`` ends the stream (a new one starts).  Returns
        ``busy`` afterwards."""
        x = np.concatenate([self.carry, np.asarray(samples, np.int16)])
        nblk = x.size // BLOCK
        for b in range(nblk):
            amp = int(np.abs(x[b * BLOCK:(b + 1) * BLOCK].astype(np.int64)).sum()) >> 11
            if self.mode == 0:
                self.mode = 1                               # ref:303
            elif self.mode == 1:
                if amp > self.amp_start:                    # ref:306-309
                    self.mode = 2
            elif amp < self.amp_end:                        # ref:316-318 (the block is still recorded)
                self.mode = 0
        self.carry = x[nblk * BLOCK:]
        self.pos += np.asarray(samples).size
        if flush:
            self.reset()
        return self.busy


def busy_after(capture, sizes, amp_start: int = 18000, amp_end: int = 14000) -> list:
    """``busy`` after each push of ``sizes`` samples of one channel's ``capture``."""
    m, p, out = BusyModel(amp_start, amp_end), 0, []
    for t in sizes:
        out.append(m.push(capture[p: p + t]))
        p += t
    return out
