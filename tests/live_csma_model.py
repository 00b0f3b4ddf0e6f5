"""A pure-Python model of the half-duplex additions of the live side (afsk_live_tx_pull_csma, afsk_live_push_muted,
``LiveTransmitter.pull(persist=, slot=, seed=)``, ``LiveReceiver.push(mute=)``), written from the header's rules alone:

* ``hash32`` / ``slots_drawn``: the counter hash and the draw G of a held channel.
* ``CsmaTxModel`` / ``CsmaTxRatedModel``: the hold models (tests/live_tx_hold_model.py, imported, not edited) with the
  modified step 5 -- a held channel's wait is ``holdoff + slot * G`` and its draw counter goes up -- and ``on_air``.
* ``mute_ranges`` / ``muted``: the clamped column ranges of a muted push and the chunk with them zeroed; the gate and
  stream models then run on that chunk as on any other.
* ``SharedChannel``: two stations and a third burst on one medium, tick by tick, for the collision scenario.

tests/test_live_csma_host.py pins them against hand-worked cases; tests/test_gpu_live_csma.py uses them as the expected
value.  They never see a kernel's output.  Not a test module."""
from __future__ import annotations

import numpy as np

from tests import live_tx_hold_model as H
from tests.live_tx_model import TAIL

M32 = 0xFFFFFFFF
SLOT_MAX = 1 << 20


def hash32(x):
    """The noise generator's hash on uint32 (a Python int or a numpy array of any integer type)."""
    x = np.asarray(x, np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x if x.ndim else int(x)


def draw_base(seed, c, k):
    """base of channel c's k-th draw (c and k may be arrays)."""
    c = (np.asarray(c, np.uint64) + np.uint64(0x9E3779B9)) & np.uint64(M32)
    inner = np.asarray(hash32(np.uint64(int(seed) & M32) ^ np.asarray(hash32(c), np.uint64)), np.uint64)
    return hash32(inner ^ (np.asarray(k, np.uint64) & np.uint64(M32)))


def slots_drawn(seed, c, k, persist, h=hash32):
    """G: the smallest j in 0 ... 254 with (h(base ^ j) & 255) <= persist, 255 when there is none."""
    base = int(draw_base(seed, c, k))
    for j in range(255):
        if (int(h(base ^ j)) & 255) <= persist:
            return j
    return 255


def slots_drawn_many(seed, c, k, persist):
    """``slots_drawn`` for arrays c and k (broadcast), as an int64 array."""
    base = np.asarray(draw_base(seed, c, k), np.uint64)
    g = np.full(base.shape, 255, np.int64)
    for j in range(254, -1, -1):
        hit = (np.asarray(hash32(base ^ np.uint64(j)), np.uint64) & np.uint64(255)) <= np.uint64(persist)
        g[hit] = j
    return g


def on_air_of(queue, pos: int, L: int):
    """(lo, hi): the hull, relative to pos, of the tones [start, start + n - TAIL) of ``queue``'s (start, n) messages
    inside [pos, pos + L); (0, 0) when there are none."""
    lo = hi = None
    for s, n in queue:
        a, b = max(s, pos), min(s + n - TAIL, pos + L)
        if b > a:
            lo = a if lo is None else min(lo, a)
            hi = b if hi is None else max(hi, b)
    return (0, 0) if lo is None else (lo - pos, hi - pos)


class _CsmaRule:
    """``pull_csma`` over a hold model.  ``channel_ids``: the transmitter channel of every model row (the draw is keyed
    by it; None: row r is channel r)."""

    def __init__(self, *args, channel_ids=None, **kw):
        super().__init__(*args, **kw)
        self.draws = [0] * self.n                           # k: 0 after create
        self.channel_ids = list(range(self.n)) if channel_ids is None else [int(c) for c in channel_ids]

    def pull_csma(self, T: int, lens=None, hold=None, holdoff: int = 0, persist: int = 255, slot: int = 0,
                  seed: int = 0, fill: int = 0):
        """One csma pull: ``(samples, pending, deferred, on_air int32 [n, 2])``.  Steps 1-4 are the hold model's; what
        it shifted follows from its ``deferred`` (the messages with start >= pos moved by it), so ``on_air`` is read
        from the queue before the pull with that shift applied."""
        assert 0 <= persist <= 255 and 0 <= slot <= SLOT_MAX
        L = [T if lens is None else min(max(int(lens[c]), 0), T) for c in range(self.n)]
        held = [bool(hold[c]) if hold is not None else False for c in range(self.n)]
        before = [(self.pos[c], list(self.queue[c])) for c in range(self.n)]
        out, pending, deferred = self.pull_hold(T, lens, hold, holdoff, fill)
        on_air = np.zeros((self.n, 2), np.int32)
        for c, (pos, q) in enumerate(before):
            shifted = [(s + int(deferred[c]) if s >= pos else s, n) for s, n in q]
            on_air[c] = on_air_of(shifted, pos, L[c])
            if held[c]:                                     # step 5, held: the hold model has set w = holdoff
                self.wait[c] = int(holdoff) + int(slot) * slots_drawn(seed, self.channel_ids[c], self.draws[c], persist)
                assert self.wait[c] < 2 ** 31
                self.draws[c] = (self.draws[c] + 1) & M32
        return out, pending, deferred, on_air

    def reset(self, mask=None) -> None:
        super().reset(mask)
        for c in range(self.n):
            if mask is None or mask[c]:
                self.draws[c] = 0


class CsmaTxModel(_CsmaRule, H.HoldTxModel):
    """``HoldTxModel`` (one geometry) with ``pull_csma``."""


class CsmaTxRatedModel(_CsmaRule, H.HoldTxRatedModel):
    """``HoldTxRatedModel`` (a geometry per message out of a table) with ``pull_csma``."""


# ------------------------------------------------------------------------------------------------------- mute

def mute_ranges(mute, lens, T: int) -> np.ndarray:
    """int64 [n, 2]: (lo', hi') per channel -- lo' = clamp(mute[c][0], 0, len_c), hi' = clamp(mute[c][1], lo', len_c)
    with len_c = clamp(lens[c], 0, T) (``lens`` None: T)."""
    mute = np.asarray(mute, np.int64)
    n = mute.shape[0]
    ln = np.full(n, T, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 0, T)
    lo = np.clip(mute[:, 0], 0, ln)
    hi = np.clip(mute[:, 1], lo, ln)
    return np.stack([lo, hi], axis=1)


def muted(chunk, mute, lens=None) -> np.ndarray:
    """A copy of ``chunk`` ([n, T]) with every channel's muted columns zeroed: what the muted push hears."""
    out = np.array(chunk, copy=True)
    for c, (lo, hi) in enumerate(mute_ranges(mute, lens, out.shape[1])):
        out[c, lo:hi] = 0
    return out


# ---------------------------------------------------------------------------------------------- the shared channel

class SharedChannel:
    """``pairs`` media, each shared by channel c of station A, channel c of station B and a third sender whose samples
    are given (``third`` [pairs, ticks * T]).  A tick: every station pushes the medium's last T samples into its gate
    (``BusyModel``, one per channel; with ``mute`` the columns its own last pull had on air zeroed first), then pulls
    T samples with hold = busy; the medium's next T samples are the third sender's plus both pulls, clipped to int16.
    ``monitor[c]`` collects the medium.  The stations are ``CsmaTxModel``s with ``seeds[s]``."""

    def __init__(self, stations, third, T: int, holdoff: int, persist: int, slot: int, seeds, mute: bool = True,
                 amp_start: int = 18000, amp_end: int = 14000):
        self.st, self.third, self.T = stations, np.asarray(third, np.int16), int(T)
        self.kw = [dict(holdoff=holdoff, persist=persist, slot=slot, seed=s) for s in seeds]
        self.n = self.third.shape[0]
        self.mute = mute
        self.gates = [[H.BusyModel(amp_start, amp_end) for _ in range(self.n)] for _ in stations]
        self.last = [np.zeros((self.n, self.T), np.int16) for _ in stations]      # every station's last pull
        self.on_air = [np.zeros((self.n, 2), np.int32) for _ in stations]
        self.t = 0
        self.medium = []

    def chunk(self) -> np.ndarray:
        """The medium's T samples of this tick."""
        t0 = self.t * self.T
        x = self.third[:, t0: t0 + self.T].astype(np.int64)
        for p in self.last:
            x = x + p
        return np.clip(x, -32768, 32767).astype(np.int16)

    def tick(self):
        """``(chunk, [heard per station], [busy per station], [(samples, pending, deferred, on_air) per station])``."""
        chunk = self.chunk()
        self.medium.append(chunk)
        heard, busy, pulls = [], [], []
        for s, st in enumerate(self.st):
            x = muted(chunk, self.on_air[s]) if self.mute else chunk
            heard.append(x)
            busy.append([g.push(x[c]) for c, g in enumerate(self.gates[s])])
        for s, st in enumerate(self.st):
            pulls.append(st.pull_csma(self.T, hold=busy[s], **self.kw[s]))
            self.last[s], self.on_air[s] = pulls[-1][0], pulls[-1][3]
        self.t += 1
        return chunk, heard, busy, pulls
