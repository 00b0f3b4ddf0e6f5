"""A pure-Python model of the rated live transmitter's queues (afsk_live_tx_create_rated, ``LiveTransmitter(n,
rates=[...])``): ``LiveTxModel`` (tests/live_tx_model.py) with a geometry per MESSAGE out of a table and the
``LIVE_TX_BAD_RATE`` rule, and the relay rule of ``afsk_live_tx_submit_events_rated`` -- the rate of a record is what
the receiver's push left at (channel, slot) -- written from the header's rules alone.

tests/test_live_tx_rated_host.py pins it against hand-worked cases; tests/test_gpu_live_tx_rated.py uses it as the
expected value.  It never sees a kernel's output.  Not a test module."""
from __future__ import annotations

import numpy as np

from afskmodem_amd import _native
from tests import live_relay_model as R
from tests.live_tx_model import TAIL, LiveTxModel

BAD_RATE = _native.LIVE_TX_BAD_RATE


class LiveTxRatedModel(LiveTxModel):
    """``table``: [(bit_frames, ts_cycles), ...].  ``wav(payload, entry)`` -> the .wav samples of a message at table
    entry ``entry`` (only for ``expected``)."""

    def __init__(self, n_channels: int, table, queue_depth: int, max_payload_len: int, wav=None):
        super().__init__(n_channels, 0, 0, queue_depth, max_payload_len,
                         None if wav is None else (lambda pe: wav(pe[0], pe[1])))
        self.table = [(int(bf), max(int(ts), 0)) for bf, ts in table]

    def n_samples(self, plen: int, entry: int = 0) -> int:
        bf, ts = self.table[entry]
        return bf * (2 * ts + 4 + 14 * plen) + TAIL

    def entry_of(self, bit_frames: int) -> int:
        """The first table entry with ``bit_frames``; ``len(table)`` -- no entry -- when there is none."""
        return next((k for k, (bf, _) in enumerate(self.table) if bf == bit_frames), len(self.table))

    def submit(self, channels, payloads, rate_index=None, sort: bool = True):
        """``LiveTxModel.submit`` with the table entry of every message (None: entry 0).  The checks of a message run
        in this order: UNSORTED, BAD_CHANNEL, TOO_LONG, BAD_RATE, QUEUE_FULL."""
        payloads = [p.encode() if isinstance(p, str) else bytes(p) for p in payloads]
        ch = [int(c) for c in channels]
        m = len(payloads)
        rate = [0] * m if rate_index is None else [int(r) for r in rate_index]
        status, start, ns = [0] * m, [-1] * m, [0] * m
        if sort:
            order = sorted(range(m), key=lambda i: ch[i] if 0 <= ch[i] < self.n else -1)
            first_bad = m
        else:
            order = list(range(m))
            first_bad = next((i for i in range(1, m) if ch[i] < ch[i - 1]), m)
        for k, i in enumerate(order):
            c, p, r = ch[i], payloads[i], rate[i]
            if k >= first_bad:
                status[i] = _native.LIVE_TX_UNSORTED
            elif not 0 <= c < self.n:
                status[i] = _native.LIVE_TX_BAD_CHANNEL
            elif len(p) > self.max_payload:
                status[i] = _native.LIVE_TX_TOO_LONG
            elif not 0 <= r < len(self.table):
                status[i] = BAD_RATE
            elif len(self.queue[c]) >= self.depth:
                status[i] = _native.LIVE_TX_QUEUE_FULL
            else:
                s, n = max(self.pos[c], self.end[c]), self.n_samples(len(p), r)
                self.queue[c].append((s, n))
                self.on_air[c].append((s, n, (p, r)))
                self.end[c] = s + n
                status[i], start[i], ns[i] = _native.LIVE_TX_QUEUED, s, n
        return np.array(status, np.int32), np.array(start, np.int64), np.array(ns, np.int32)

    def expected_ragged(self, T: int, lens, fill: int = 0) -> np.ndarray:
        """``expected(T)`` of a ragged pull into a buffer that held ``fill``: columns from clamp(lens[c], 0, T) on
        are untouched."""
        out = self.expected(T)
        for c in range(self.n):
            out[c, min(max(int(lens[c]), 0), T):] = fill
        return out

    def pull_ragged(self, T: int, lens) -> np.ndarray:
        """Advance channel c by clamp(lens[c], 0, T), retire what ended; returns pending."""
        for c in range(self.n):
            self.pos[c] += min(max(int(lens[c]), 0), T)
            q = self.queue[c]
            while q and q[0][0] + q[0][1] <= self.pos[c]:
                q.popleft()
            self.on_air[c] = [e for e in self.on_air[c] if e[0] + e[1] > self.pos[c]]
        return self.pending()


def relay_heard(tx_model: LiveTxRatedModel, buf, max_events: int, max_bytes: int, out_stride: int, n_rx: int, rx_bf,
                channel_map=None, skip_flags: int = R.OPEN_END):
    """``(status, start, n_samples, queued)`` of ``afsk_live_tx_submit_events_rated``: ``live_relay_model.relay`` with
    the rate of record r read from ``rx_bf[r.channel, r.slot]`` (int32 [n_rx, slots]).  A record with no place in that
    array is SKIPPED (among the SKIPPED conditions: before any channel rule); a rate the table lacks is BAD_RATE behind
    BAD_CHANNEL and TOO_LONG, in front of QUEUE_FULL.  ``queued``: (destination, payload, table entry) handed on."""
    rx_bf = np.asarray(rx_bf, np.int32)
    assert rx_bf.ndim == 2 and rx_bf.shape[0] == n_rx
    header, recs, payload = R.parts(buf, max_events, max_bytes)
    stored = min(max(int(header["stored"]), 0), max_events)
    status = np.full(max_events, R.NONE, np.int32)
    start = np.full(max_events, -1, np.int64)
    ns = np.zeros(max_events, np.int32)
    ch = recs["channel"][:stored].astype(np.int64)
    first_bad = next((i for i in range(1, stored) if ch[i] < ch[i - 1]), stored)
    status[first_bad:stored] = R.UNSORTED
    at, dsts, pays, entries = [], [], [], []
    for i in range(first_bad):
        r = recs[i]
        nb, off, slot = int(r["nbytes"]), int(r["payload_offset"]), int(r["slot"])
        if (int(r["flags"]) & (R.OVERFLOW | skip_flags)) or int(r["status"]) != _native.ST_OK or nb < 1 \
                or nb > out_stride or off < 0 or off + nb > max_bytes \
                or not 0 <= int(ch[i]) < n_rx or not 0 <= slot < rx_bf.shape[1]:
            status[i] = R.SKIPPED
            continue
        dst = int(ch[i])
        if channel_map is not None:
            dst = int(channel_map[dst])
            if dst < 0:
                status[i] = R.SKIPPED
                continue
        if not 0 <= dst < tx_model.n:
            status[i] = R.BAD
            continue
        at.append(i)
        dsts.append(dst)
        pays.append(payload[off: off + nb].tobytes())
        entries.append(tx_model.entry_of(int(rx_bf[int(ch[i]), slot])))
    if at:
        st, s, n = tx_model.submit(dsts, pays, entries)
        status[at], start[at], ns[at] = st, s, n
    return status, start, ns, list(zip(dsts, pays, entries))
