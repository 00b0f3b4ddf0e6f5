"""A pure-Python model of the duplicate filter (``afsk_live_dedup_*``, ``afsk_live_tx_submit_events_kept``,
include/afsk_amd.h), written from its rules alone: the key in Python ints, the table in numpy arrays laid out as
``LiveDedup.state`` returns them, filter, note, reset, and the relay with a ``keep`` array on top of
tests/live_relay_model.py's.

tests/test_live_dedup_host.py pins it against hand-worked cases; tests/test_gpu_live_dedup.py uses it as the expected
value.  It never sees a kernel's output.  Not a test module."""
from __future__ import annotations

import numpy as np

from afskmodem_amd import _native
from tests import live_events_model as M
from tests import live_relay_model as R

NONE, DUP, NEW, PASS = -1, 0, 1, 2                       # AFSK_LIVE_DEDUP_*
DUPLICATE = 7                                            # AFSK_LIVE_TX_DUPLICATE
EMPTY = -(2 ** 63)
MASK = (1 << 64) - 1
ENTRY = np.dtype([("key", "<u8"), ("time", "<i8")])
OPEN_END, OVERFLOW = _native.LIVE_OPEN_END, _native.LIVE_OVERFLOW


def mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def key(p: bytes) -> int:
    """The key of a payload: mix64((sum of mix64(i << 8 | p[i])) ^ (n << 32)), all mod 2^64."""
    s = 0
    for i, b in enumerate(bytes(p)):
        s = (s + mix64((i << 8) | b)) & MASK
    return mix64(s ^ ((len(p) << 32) & MASK))


def keys_np(rows: np.ndarray) -> np.ndarray:
    """``key`` of every row of a uint8 [n, length] matrix at once (numpy's uint64 arithmetic wraps mod 2^64)."""
    def mix(z):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    n, length = rows.shape
    with np.errstate(over="ignore"):
        terms = mix((np.arange(length, dtype=np.uint64)[None, :] << np.uint64(8)) | rows.astype(np.uint64))
        return mix(terms.sum(axis=1, dtype=np.uint64) ^ np.uint64(length << 32))


def wrap64(t: int) -> int:
    """``t`` as an int64 holds it (burst_start + burst_len wraps like the device's addition)."""
    t &= MASK
    return t - (1 << 64) if t >= 1 << 63 else t


def events_buffer(rows, max_events: int, max_bytes: int, payload: bytes, stored=None, fill=0x5A) -> np.ndarray:
    """An events buffer (without the scratch) of the records ``rows`` -- (channel, burst_start, burst_len, flags, status,
    nbytes, payload_offset) each -- over the payload part ``payload``; ``stored``: the header's, len(rows) when None."""
    if isinstance(rows, np.ndarray) and rows.dtype == M.EVENT:           # (the records themselves)
        recs = rows
    else:
        recs = np.zeros(len(rows), M.EVENT)
        for i, (ch, start, ln, fl, st, nb, off) in enumerate(rows):
            recs[i] = (ch, 0, start, ln, fl, st, nb, 8 * nb, 0, 0, off)
    n = len(rows) if stored is None else stored
    h = np.array([(n, n, len(payload), len(payload), 0)], M.HEADER)
    out = np.full(M.HEADER.itemsize + M.EVENT.itemsize * max_events + max_bytes, fill, np.uint8)
    out[: M.HEADER.itemsize] = h.view(np.uint8)
    keep = min(len(rows), max_events)
    out[M.HEADER.itemsize: M.HEADER.itemsize + M.EVENT.itemsize * keep] = recs[:keep].view(np.uint8)
    at = M.HEADER.itemsize + M.EVENT.itemsize * max_events
    pay = np.frombuffer(bytes(payload), np.uint8)[:max_bytes]
    out[at: at + pay.size] = pay
    return out


def eligible(r, n_channels: int, max_bytes: int, out_stride: int, skip_flags: int) -> bool:
    nb, off = int(r["nbytes"]), int(r["payload_offset"])
    return 0 <= int(r["channel"]) < n_channels and int(r["status"]) == _native.ST_OK and 1 <= nb <= out_stride \
        and off >= 0 and off + nb <= max_bytes and not int(r["flags"]) & (skip_flags | OVERFLOW)


class DedupModel:
    def __init__(self, n_channels: int, depth: int):
        self.n, self.depth = n_channels, depth
        self.entries = np.zeros((n_channels, depth), ENTRY)
        self.entries["time"] = EMPTY
        self.head = np.zeros(n_channels, np.int32)

    def copy(self) -> "DedupModel":
        m = DedupModel(self.n, self.depth)
        m.entries, m.head = self.entries.copy(), self.head.copy()
        return m

    def look(self, ch: int, k: int, t: int, window: int) -> int:
        """One eligible item of channel ``ch``: DUP, or NEW with the insertion made."""
        for e in self.entries[ch]:
            et = int(e["time"])
            if et != EMPTY and int(e["key"]) == k and 0 <= t - et < window:
                return DUP
        self.entries[ch, self.head[ch]] = (k, t)
        self.head[ch] = (self.head[ch] + 1) % self.depth
        return NEW

    def filter(self, buf, max_events: int, max_bytes: int, out_stride: int, window: int,
               skip_flags: int = OPEN_END) -> np.ndarray:
        header, recs, payload = R.parts(buf, max_events, max_bytes)
        stored = min(max(int(header["stored"]), 0), max_events)
        verdict = np.full(max_events, NONE, np.int32)
        ch = recs["channel"][:stored].astype(np.int64)
        first_bad = next((i for i in range(1, stored) if ch[i] < ch[i - 1]), stored)
        verdict[first_bad:stored] = PASS
        for i in range(first_bad):
            r = recs[i]
            if not eligible(r, self.n, max_bytes, out_stride, skip_flags):
                verdict[i] = PASS
                continue
            off, nb = int(r["payload_offset"]), int(r["nbytes"])
            t = wrap64(int(r["burst_start"]) + int(r["burst_len"]))
            verdict[i] = self.look(int(r["channel"]), key(payload[off: off + nb].tobytes()), t, window)
        return verdict

    def note(self, channels, payloads, times, window: int, payload_stride=None) -> np.ndarray:
        """The C entry's rule: ``channels`` as given (at or past the first descending one: PASS)."""
        n = len(payloads)
        stride = max([len(p) for p in payloads] + [1]) if payload_stride is None else payload_stride
        verdict = np.full(n, PASS, np.int32)
        first_bad = next((i for i in range(1, n) if channels[i] < channels[i - 1]), n)
        for i in range(first_bad):
            if 0 <= channels[i] < self.n and 1 <= len(payloads[i]) <= stride:
                verdict[i] = self.look(int(channels[i]), key(payloads[i]), int(times[i]), window)
        return verdict

    def note_any_order(self, channels, payloads, times, window: int) -> np.ndarray:
        """``LiveDedup.note`` on host lists: sorted by channel (stable, a channel outside the filter's first), the
        verdicts back in list order."""
        ch = [c if 0 <= c < self.n else -1 for c in channels]
        order = sorted(range(len(ch)), key=lambda i: ch[i])
        v = self.note([ch[i] for i in order], [payloads[i] for i in order], [times[i] for i in order], window)
        out = np.zeros(len(ch), np.int32)
        out[order] = v
        return out

    def reset(self, mask=None) -> None:
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        self.entries["key"][sel] = 0
        self.entries["time"][sel] = EMPTY
        self.head[sel] = 0


def relay_kept(tx_model, buf, max_events: int, max_bytes: int, out_stride: int, n_rx: int, keep, channel_map=None,
               skip_flags: int = OPEN_END):
    """tests/live_relay_model.py's ``relay`` with a ``keep`` entry per record: a relayable record whose entry is 0 answers
    DUPLICATE -- behind the SKIPPED conditions, in front of BAD_CHANNEL -- and is not handed to the queue model."""
    header, recs, payload = R.parts(buf, max_events, max_bytes)
    stored = min(max(int(header["stored"]), 0), max_events)
    status = np.full(max_events, R.NONE, np.int32)
    start = np.full(max_events, -1, np.int64)
    ns = np.zeros(max_events, np.int32)
    ch = recs["channel"][:stored].astype(np.int64)
    first_bad = next((i for i in range(1, stored) if ch[i] < ch[i - 1]), stored)
    status[first_bad:stored] = R.UNSORTED
    at, dsts, pays = [], [], []
    for i in range(first_bad):
        r = recs[i]
        nb, off = int(r["nbytes"]), int(r["payload_offset"])
        dst = int(ch[i])
        dropped = channel_map is not None and 0 <= dst < n_rx and int(channel_map[dst]) < 0
        if (int(r["flags"]) & (OVERFLOW | skip_flags)) or int(r["status"]) != _native.ST_OK or nb < 1 \
                or nb > out_stride or off < 0 or off + nb > max_bytes or dropped:
            status[i] = R.SKIPPED
            continue
        if int(keep[i]) == 0:
            status[i] = DUPLICATE
            continue
        if channel_map is not None:
            dst = int(channel_map[dst]) if 0 <= dst < n_rx else -1
        if not 0 <= dst < tx_model.n:
            status[i] = R.BAD
            continue
        at.append(i)
        dsts.append(dst)
        pays.append(payload[off: off + nb].tobytes())
    if at:
        st, s, n = tx_model.submit(dsts, pays)
        status[at], start[at], ns[at] = st, s, n
    return status, start, ns, list(zip(dsts, pays))
