"""A pure-Python model of the relay submit (``afsk_live_tx_submit_events``, include/afsk_amd.h), written from its rules
alone.  It reads an events buffer as the numpy model packs it (tests/live_events_model.py: ``buffer``), decides per
record place -- NONE, UNSORTED, SKIPPED, BAD_CHANNEL -- and hands the relayable records' destination channels and
payloads, in record order, to ``LiveTxModel.submit`` (tests/live_tx_model.py), which decides the rest: TOO_LONG,
QUEUE_FULL or QUEUED with its start and sample count.

tests/test_live_relay_host.py pins it against hand-worked cases; tests/test_gpu_live_relay.py uses it as the expected
value.  It never sees a kernel's output.  Not a test module."""
from __future__ import annotations

import numpy as np

from afskmodem_amd import _native
from tests import live_events_model as M

NONE, SKIPPED = _native.LIVE_TX_NONE, _native.LIVE_TX_SKIPPED
BAD, UNSORTED = _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED
OPEN_END, OVERFLOW = _native.LIVE_OPEN_END, _native.LIVE_OVERFLOW


def parts(buf, max_events: int, max_bytes: int):
    """``(header, records [max_events], payload part [max_bytes])`` of an events buffer (a numpy uint8 array)."""
    buf = np.ascontiguousarray(buf, np.uint8)
    at = M.HEADER.itemsize + M.EVENT.itemsize * max_events
    return (buf[: M.HEADER.itemsize].view(M.HEADER)[0], buf[M.HEADER.itemsize: at].view(M.EVENT),
            buf[at: at + max_bytes])


def relay(tx_model, buf, max_events: int, max_bytes: int, out_stride: int, n_rx: int, channel_map=None,
          skip_flags: int = OPEN_END):
    """``(status, start, n_samples, queued)``: the three outputs, [max_events] each, of a relay submit of the events
    buffer ``buf`` on the transmitter ``tx_model`` (a ``LiveTxModel``, which advances), and ``queued``, the
    ``(destination channel, payload)`` handed to ``tx_model.submit``, in record order."""
    header, recs, payload = parts(buf, max_events, max_bytes)
    stored = min(max(int(header["stored"]), 0), max_events)
    status = np.full(max_events, NONE, np.int32)
    start = np.full(max_events, -1, np.int64)
    ns = np.zeros(max_events, np.int32)
    ch = recs["channel"][:stored].astype(np.int64)
    first_bad = next((i for i in range(1, stored) if ch[i] < ch[i - 1]), stored)
    status[first_bad:stored] = UNSORTED
    at, dsts, pays = [], [], []
    for i in range(first_bad):
        r = recs[i]
        nb, off = int(r["nbytes"]), int(r["payload_offset"])
        if (int(r["flags"]) & (OVERFLOW | skip_flags)) or int(r["status"]) != _native.ST_OK or nb < 1 \
                or nb > out_stride or off < 0 or off + nb > max_bytes:
            status[i] = SKIPPED
            continue
        dst = int(ch[i])
        if channel_map is not None:
            if not 0 <= dst < n_rx:
                status[i] = BAD
                continue
            dst = int(channel_map[dst])
            if dst < 0:
                status[i] = SKIPPED
                continue
        if not 0 <= dst < tx_model.n:
            status[i] = BAD
            continue
        at.append(i)
        dsts.append(dst)
        pays.append(payload[off: off + nb].tobytes())
    if at:
        # (a stable sort by channel keeps every channel's record order, and the channels' queues are independent)
        st, s, n = tx_model.submit(dsts, pays)
        status[at], start[at], ns[at] = st, s, n
    return status, start, ns, list(zip(dsts, pays))
