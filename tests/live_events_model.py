"""A numpy reference of the packed event list of a live push (``afsk_live_pack``, include/afsk_amd.h), written from its
rules alone: channel c reports ``clamp(n_closed[c], 0, slots)`` bursts; record order is channel ascending, then slot
ascending; a record keeps ``min(max(nbytes, 0), out_stride)``
bytes of its row, none with ``AFSK_LIVE_OVERFLOW``; its ``payload_offset`` is the sum of the kept bytes of all records
before it, or -1 when that sum plus its own kept bytes exceeds ``max_bytes`` (then the payload is not written); records
from index ``max_events`` on are not written, nor are their payloads; the header counts everything all the same.

``pack`` walks the records in Python and is the plain statement of the rules; ``pack_fast`` is the same function of the
same arrays by cumulative sums, for pushes of more channels and wider rows than a Python loop or a host copy of the rows
could take (tests/test_live_events_host.py holds the two equal, field for field and byte for byte).

It is the expected value of the GPU tests and the source of the hand-built buffers of the host tests.  It never sees a
kernel's output."""
import numpy as np

OVERFLOW = 2                                                    # AFSK_LIVE_OVERFLOW
HEADER = np.dtype([("count", "<i4"), ("stored", "<i4"), ("n_bytes", "<i8"), ("stored_bytes", "<i8"), ("reserved", "<i8")])
EVENT = np.dtype([("channel", "<i4"), ("slot", "<i4"), ("burst_start", "<i8"), ("burst_len", "<i4"), ("flags", "<i4"),
                  ("status", "<i4"), ("nbytes", "<i4"), ("nbits", "<i4"), ("clock_idx", "<i4"), ("term_frame", "<i4"),
                  ("payload_offset", "<i4")])
FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")


def pack(n_closed, burst_start, burst_len, flags, rows, demod, max_events, max_bytes):
    """``(header, records, payload)`` of one push: ``n_closed`` [n]; ``burst_start`` / ``burst_len`` / ``flags``
    [n, slots]; ``rows`` uint8 [n * slots, out_stride]; ``demod`` a dict of the five vectors of FIELDS, [n * slots]."""
    n, slots = burst_len.shape
    stride = rows.shape[1]
    recs, payload, count, off = [], bytearray(), 0, 0
    for c in range(n):
        for k in range(min(max(int(n_closed[c]), 0), slots)):
            r = c * slots + k
            kept = 0 if flags[c, k] & OVERFLOW else min(max(int(demod["nbytes"][r]), 0), stride)
            if count < max_events:
                fits = off + kept <= max_bytes
                recs.append((c, k, burst_start[c, k], burst_len[c, k], flags[c, k], demod["status"][r], demod["nbytes"][r],
                             demod["nbits"][r], demod["clock_idx"][r], demod["term_frame"][r], off if fits else -1))
                if fits:
                    payload += rows[r, :kept].tobytes()
            count += 1
            off += kept
    header = np.array([(count, min(count, max_events), off, len(payload), 0)], HEADER)
    return header, np.array(recs, EVENT), bytes(payload)


def pack_fast(n_closed, burst_start, burst_len, flags, rows, demod, max_events, max_bytes):
    """``pack`` without a loop over the records and without the rows' bytes: ``rows`` is the payload rows or their
    ``out_stride`` alone.  Returns ``(header, records, copies)``: the header and the records are ``pack``'s; ``copies``
    is int64 [stored, 4], per stored record ``(source row, source start, length, destination offset)`` of the payload
    bytes that are written -- ``rows[row, start : start + length]`` lands at ``destination`` of the payload part --
    with length 0 and destination -1 where the payload is not written (``gather`` makes ``pack``'s payload of it)."""
    n, slots = burst_len.shape
    stride = rows if isinstance(rows, (int, np.integer)) else rows.shape[1]
    nc = np.clip(np.asarray(n_closed, np.int64), 0, slots)
    r = np.flatnonzero((np.arange(slots)[None, :] < nc[:, None]).reshape(-1))      # channel, then slot ascending
    fl = flags.reshape(-1)[r]
    kept = np.where(fl & OVERFLOW, 0, np.clip(demod["nbytes"][r].astype(np.int64), 0, stride))
    end = np.cumsum(kept)
    off = end - kept
    count = r.size
    stored = min(count, max_events)
    fits = (end <= max_bytes)[:stored]
    recs = np.zeros(stored, EVENT)
    s = r[:stored]
    recs["channel"], recs["slot"] = s // slots, s % slots
    recs["burst_start"], recs["burst_len"], recs["flags"] = burst_start.reshape(-1)[s], burst_len.reshape(-1)[s], fl[:stored]
    for f in FIELDS:
        recs[f] = demod[f][s]
    recs["payload_offset"] = np.where(fits, off[:stored], -1)
    copies = np.stack([s, np.zeros(stored, np.int64), np.where(fits, kept[:stored], 0),
                       np.where(fits, off[:stored], -1)], axis=1).astype(np.int64).reshape(stored, 4)
    header = np.array([(count, stored, int(end[-1]) if count else 0, int(copies[:, 2].sum()), 0)], HEADER)
    return header, recs, copies


def gather(rows, copies):
    """The bytes a list of ``copies`` (``pack_fast``) writes, in the order of their destinations: the written payload
    part.  The written runs lie back to back from 0 on."""
    c = copies[copies[:, 2] > 0]
    end = np.cumsum(c[:, 2])
    assert np.array_equal(c[:, 3], end - c[:, 2])
    within = np.arange(int(end[-1]) if c.size else 0) - np.repeat(end - c[:, 2], c[:, 2])
    return rows[np.repeat(c[:, 0], c[:, 2]), np.repeat(c[:, 1], c[:, 2]) + within].tobytes()


def buffer(header, records, payload, max_events, max_bytes, fill=0x5A):
    """The events buffer a pack of these capacities leaves behind, without the scratch: header, ``max_events`` record
    places, ``max_bytes`` payload places; what was not written holds ``fill``."""
    out = np.full(HEADER.itemsize + EVENT.itemsize * max_events + max_bytes, fill, np.uint8)
    out[: HEADER.itemsize] = header.view(np.uint8)
    out[HEADER.itemsize: HEADER.itemsize + records.nbytes] = records.view(np.uint8)
    at = HEADER.itemsize + EVENT.itemsize * max_events
    out[at: at + len(payload)] = np.frombuffer(payload, np.uint8)
    return out


def random_push(rng, n, slots, stride, pattern, marker=0xEE, uniform=False):
    """Hand-made outputs of one push.  ``pattern``: which channels report bursts ("zero", "full", "sparse", "last",
    "first", "wild").  ``nbytes`` comes from {0, 1, 3, stride - 1, stride, stride + 5} (``uniform``: from all of
    0 ... stride + 5), some records carry OVERFLOW, and every row byte a pack may not copy -- the rows of unused slots,
    and used rows past their kept bytes -- is ``marker``, which no kept byte equals.  The slot arrays of unused slots
    hold values a pack would visibly mis-pack.  "wild" is "sparse" with ``n_closed`` outside its range where a channel
    reports: -3 ... -1 (nothing counts, and the slot arrays say so) or slots + 1 ... slots + 3 (every slot counts, none
    beyond), to meet the clamp."""
    wild = None
    if pattern == "wild":
        nc = np.where(rng.integers(0, 16, n) == 0, rng.integers(1, slots + 1, n), 0).astype(np.int32)
        wild = np.where(nc > 0, rng.integers(0, 3, n), 0)          # 1: below the range; 2: above it
        nc = np.where(wild == 1, 0, np.where(wild == 2, slots, nc)).astype(np.int32)
    elif pattern == "zero":
        nc = np.zeros(n, np.int32)
    elif pattern == "full":
        nc = np.full(n, slots, np.int32)
    elif pattern == "sparse":
        nc = np.where(rng.integers(0, 16, n) == 0, rng.integers(1, slots + 1, n), 0).astype(np.int32)
    else:
        nc = np.zeros(n, np.int32)
        nc[-1 if pattern == "last" else 0] = rng.integers(1, slots + 1)
    used = np.arange(slots)[None, :] < nc[:, None]
    m = n * slots
    start = np.where(used, rng.integers(0, 1 << 40, (n, slots)) * 2048, -7).astype(np.int64)
    length = np.where(used, rng.integers(1, 64, (n, slots)) * 2048, -7).astype(np.int32)
    flags = np.where(used, rng.choice([0, 0, 0, 1, 2, 3], (n, slots)), 0x7fff).astype(np.int32)
    demod = {f: np.where(used.reshape(-1), rng.integers(-50, 1 << 20, m), 0x7fffffff).astype(np.int32) for f in FIELDS}
    drawn = rng.integers(0, stride + 6, m) if uniform else rng.choice([0, 1, 3, stride - 1, stride, stride + 5], m)
    demod["nbytes"] = np.where(used.reshape(-1), drawn, 0x7fffffff).astype(np.int32)
    kept = np.where(used.reshape(-1), np.clip(demod["nbytes"], 0, stride), 0)
    rows = rng.integers(0, marker, (m, stride), dtype=np.uint8)
    rows[np.arange(stride)[None, :] >= kept[:, None]] = marker
    if wild is not None:
        nc = np.where(wild == 1, -rng.integers(1, 4, n), np.where(wild == 2, slots + rng.integers(1, 4, n), nc))
        nc = nc.astype(np.int32)
    return nc, start, length, flags, rows, demod


def slot_bursts(n_closed, burst_start, burst_len, flags, rows, demod):
    """``(channel, start, length, payload)`` per reported burst straight from the slot arrays: what
    ``LiveResult.bursts()`` lists."""
    n, slots = burst_len.shape
    out = []
    for c in range(n):
        for k in range(min(max(int(n_closed[c]), 0), slots)):
            r = c * slots + k
            kept = 0 if flags[c, k] & OVERFLOW else min(max(int(demod["nbytes"][r]), 0), rows.shape[1])
            out.append((c, int(burst_start[c, k]), int(burst_len[c, k]), rows[r, :kept].tobytes()))
    return out
