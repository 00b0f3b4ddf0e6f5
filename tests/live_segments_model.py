"""A numpy reference of the packed segment list of a progressive live push (``afsk_live_pack_tap``,
include/afsk_amd.h), written from its rules alone.

The per-channel rule.  For channel c: ``nc = clamp(n_closed[c], 0, slots)``, ``tn = clamp(tap_n[c], 0, tap_cap)``; with
``at = 0``, every slot ``k < nc`` in turn takes ``ln_k = clamp(tap_len[c, k], 0, tn - at)`` bytes, ``at += ln_k``;
``rest = tn - at``.  The channel has an open segment iff ``rest > 0`` and ``open_start[c] >= 0``.  It contributes ``nc``
final records ``(c, k, burst_start[c, k], burst_len[c, k], flags[c, k], nbytes[c * slots + k] - ln_k, ln_k)`` and then,
if it has one, the open record ``(c, -1, open_start[c], 0, 0, open_nbytes[c] - rest, rest)``; their data are
``tap_bytes[c, 0 : at (+ rest)]``.

The capacity rules.  Records come channel ascending, slots ascending, then the open one; the data lie back to back in
that order.  The header holds the true ``count`` and ``n_bytes``; ``stored = min(count, max_segments)``; a record's data
are written iff the record is stored and its start plus its length is at most ``max_bytes``; ``stored_bytes`` is the
start of the first record whose data are not written, or ``n_bytes`` when all are.

``pack`` walks the segments in Python and is the plain statement of the rules; ``pack_fast`` is the same function of
the same arrays by cumulative sums, for pushes of more channels and wider tap rows than a Python loop or a host copy of
the rows could take (tests/test_live_segments_host.py holds the two equal, field for field and byte for byte).

It is the expected value of the GPU tests and the source of the hand-built buffers of the host tests.  It never sees a
kernel's output."""
import numpy as np

HEADER = np.dtype([("count", "<i4"), ("stored", "<i4"), ("n_bytes", "<i8"), ("stored_bytes", "<i8"), ("reserved", "<i8")])
SEGMENT = np.dtype([("channel", "<i4"), ("slot", "<i4"), ("burst_start", "<i8"), ("burst_len", "<i4"), ("flags", "<i4"),
                    ("offset", "<i4"), ("length", "<i4")])
NAMES = ("n_closed", "burst_start", "burst_len", "flags", "nbytes", "tap_bytes", "tap_n", "tap_len", "open_start",
         "open_nbytes")
PATTERNS = ("nothing", "open_only", "all", "span_last", "random", "orphan", "wild")


def clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def i32(v):
    """``v`` as the int32 the device's 32-bit subtraction leaves."""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def segments(n_closed, burst_start, burst_len, flags, nbytes, tap_bytes, tap_n, tap_len, open_start, open_nbytes):
    """Every segment of one push, in order: ``(record tuple in SEGMENT's field order, its data)``."""
    n, slots = tap_len.shape
    cap = tap_bytes.shape[1]
    out = []
    for c in range(n):
        nc, tn, at = clamp(n_closed[c], 0, slots), clamp(tap_n[c], 0, cap), 0
        for k in range(nc):
            ln = clamp(tap_len[c, k], 0, tn - at)
            out.append(((c, k, int(burst_start[c, k]), int(burst_len[c, k]), int(flags[c, k]),
                         i32(int(nbytes[c * slots + k]) - ln), ln), tap_bytes[c, at: at + ln].tobytes()))
            at += ln
        rest = tn - at
        if rest > 0 and open_start[c] >= 0:
            out.append(((c, -1, int(open_start[c]), 0, 0, i32(int(open_nbytes[c]) - rest), rest),
                        tap_bytes[c, at: at + rest].tobytes()))
    return out


def pack(arrays, max_segments, max_bytes):
    """``(header, records, data)`` of one push's ``arrays`` (in the order of NAMES) in a buffer of these capacities."""
    segs = segments(*arrays)
    recs, data, off, stored_bytes = [], bytearray(), 0, None
    for i, (rec, seg) in enumerate(segs):
        written = i < max_segments and off + len(seg) <= max_bytes
        if i < max_segments:
            recs.append(rec)
        if written:
            assert stored_bytes is None                         # (the written data are those of the first records)
            data += seg
        elif stored_bytes is None:
            stored_bytes = off
        off += len(seg)
    if stored_bytes is None:
        stored_bytes = off
    assert stored_bytes == len(data)
    header = np.array([(len(segs), min(len(segs), max_segments), off, stored_bytes, 0)], HEADER)
    return header, np.array(recs, SEGMENT), bytes(data)


def pack_fast(arrays, max_segments, max_bytes):
    """``pack`` without a loop over the channels and without the tap bytes: ``arrays`` in the order of NAMES, where
    ``tap_bytes`` is the tap rows or their ``tap_cap`` alone.  Returns ``(header, records, copies)``: the header and the
    records are ``pack``'s; ``copies`` is int64 [stored, 4], per stored record ``(source row, source start, length,
    destination offset)`` of the data bytes that are written -- ``tap_bytes[row, start : start + length]`` lands at
    ``destination`` of the data part -- with length 0 and destination -1 where the record's data are not written
    (``gather`` makes ``pack``'s data of it)."""
    n_closed, burst_start, burst_len, flags, nbytes, tap_bytes, tap_n, tap_len, open_start, open_nbytes = arrays
    n, slots = tap_len.shape
    cap = tap_bytes if isinstance(tap_bytes, (int, np.integer)) else tap_bytes.shape[1]
    nc = np.clip(np.asarray(n_closed, np.int64), 0, slots)
    tn = np.clip(np.asarray(tap_n, np.int64), 0, cap)
    # a table of n rows and slots + 1 columns: the final segments' columns, then the open segment's
    ln = np.zeros((n, slots + 1), np.int64)
    at = np.zeros(n, np.int64)
    for k in range(slots):
        ln[:, k] = np.where(k < nc, np.clip(tap_len[:, k].astype(np.int64), 0, tn - at), 0)
        at += ln[:, k]
    has_open = (tn - at > 0) & (np.asarray(open_start) >= 0)
    ln[:, slots] = np.where(has_open, tn - at, 0)
    valid = np.concatenate([np.arange(slots)[None, :] < nc[:, None], has_open[:, None]], axis=1)
    pick = np.flatnonzero(valid.reshape(-1))                        # channel ascending, slots ascending, the open one
    c, k = pick // (slots + 1), pick % (slots + 1)
    fin = k < slots
    kf = np.where(fin, k, 0)
    length = ln.reshape(-1)[pick]
    src = (np.cumsum(ln, axis=1) - ln).reshape(-1)[pick]
    end = np.cumsum(length)
    off = end - length
    count = pick.size
    stored = min(count, max_segments)
    sl = slice(0, stored)
    recs = np.zeros(stored, SEGMENT)
    recs["channel"], recs["slot"] = c[sl], np.where(fin, k, -1)[sl]
    recs["burst_start"] = np.where(fin, burst_start[c, kf], np.asarray(open_start)[c])[sl]
    recs["burst_len"] = np.where(fin, burst_len[c, kf], 0)[sl]
    recs["flags"] = np.where(fin, flags[c, kf], 0)[sl]
    before = np.where(fin, np.asarray(nbytes, np.int64)[c * slots + kf], np.asarray(open_nbytes, np.int64)[c]) - length
    recs["offset"] = ((before + 2 ** 31) % 2 ** 32 - 2 ** 31)[sl]      # (as the device's 32-bit subtraction leaves it)
    recs["length"] = length[sl]
    written = (end <= max_bytes)[sl]
    copies = np.stack([c[sl], src[sl], np.where(written, length[sl], 0), np.where(written, off[sl], -1)],
                      axis=1).astype(np.int64).reshape(stored, 4)
    header = np.array([(count, stored, int(end[-1]) if count else 0, int(copies[:, 2].sum()), 0)], HEADER)
    return header, recs, copies


def gather(tap_bytes, copies):
    """The bytes a list of ``copies`` (``pack_fast``) writes, in the order of their destinations: the written data
    part.  The written runs lie back to back from 0 on."""
    c = copies[copies[:, 2] > 0]
    end = np.cumsum(c[:, 2])
    assert np.array_equal(c[:, 3], end - c[:, 2])
    within = np.arange(int(end[-1]) if c.size else 0) - np.repeat(end - c[:, 2], c[:, 2])
    return tap_bytes[np.repeat(c[:, 0], c[:, 2]), np.repeat(c[:, 1], c[:, 2]) + within].tobytes()


def buffer(header, records, data, max_segments, max_bytes, fill=0x5A):
    """The segments buffer a pack of these capacities leaves behind, without the scratch: header, ``max_segments``
    record places, ``max_bytes`` data places; what was not written holds ``fill``."""
    out = np.full(HEADER.itemsize + SEGMENT.itemsize * max_segments + max_bytes, fill, np.uint8)
    out[: HEADER.itemsize] = header.view(np.uint8)
    out[HEADER.itemsize: HEADER.itemsize + records.nbytes] = records.view(np.uint8)
    at = HEADER.itemsize + SEGMENT.itemsize * max_segments
    out[at: at + len(data)] = np.frombuffer(data, np.uint8)
    return out


def random_tap(rng, n, slots, cap, pattern, marker=0xEE, span=256):
    """Hand-made outputs of one tapped push, in the order of NAMES.  ``pattern``:
      nothing    no channel closed or decoded anything
      open_only  every channel has an open segment and nothing else
      all        every channel reports all its slots and has an open segment (as far as ``cap`` bytes go round)
      span_last  only the last channel of every span of ``span`` channels (and the very last channel)
      random     a random third of the channels, any mix of final segments (some of length 0) and an open one
      orphan     like random, and where bytes are left over ``open_start`` is -1: they must not come out
      wild       like random, with ``n_closed``, ``tap_n`` and ``tap_len`` outside their ranges, to meet the clamps
    Every tap byte at or past ``tap_n`` is ``marker``, which no byte before it equals; slot arrays of unused slots,
    ``tap_len`` of unused slots and ``open_start`` / ``open_nbytes`` of channels without left-over bytes hold values a
    pack would visibly mis-pack."""
    assert pattern in PATTERNS
    active = np.zeros(n, bool)
    if pattern in ("open_only", "all"):
        active[:] = True
    elif pattern == "span_last":
        active[span - 1:: span] = True
        active[-1] = True
    elif pattern != "nothing":
        active = rng.integers(0, 3, n) == 0
    nc = np.zeros(n, np.int32)
    if pattern == "all":
        nc[:] = slots
    elif pattern not in ("nothing", "open_only"):
        nc = np.where(active, rng.integers(0, slots + 1, n), 0).astype(np.int32)
    tap_len = np.full((n, slots), 0x7fffff, np.int32)
    tap_n = np.zeros(n, np.int32)
    open_start = np.full(n, 12345, np.int64)                    # (>= 0 with no bytes left over: no segment all the same)
    open_nbytes = np.full(n, 0x7fffff, np.int32)
    for c in np.nonzero(active)[0].tolist():
        left = cap
        for k in range(int(nc[c])):
            ln = int(rng.integers(0, left + 1)) if pattern != "all" else min(left, max(cap // (slots + 1), 1))
            ln = 0 if pattern != "all" and rng.integers(0, 3) == 0 else ln
            tap_len[c, k] = ln
            left -= ln
        want_open = pattern in ("open_only", "all") or rng.integers(0, 2) == 0
        rest = 0
        if want_open and left > 0:
            rest = left if pattern == "all" else int(rng.integers(1, left + 1))
        tap_n[c] = cap - left + rest
        if rest > 0:
            open_start[c] = -1 if pattern == "orphan" and rng.integers(0, 2) == 0 else int(rng.integers(0, 1 << 40)) * 2048
            open_nbytes[c] = rest + int(rng.integers(0, 1 << 16))
    tap_bytes = rng.integers(0, marker, (n, cap), dtype=np.uint8)
    tap_bytes[np.arange(cap)[None, :] >= tap_n[:, None]] = marker
    used = np.arange(slots)[None, :] < nc[:, None]
    burst_start = np.where(used, rng.integers(0, 1 << 40, (n, slots)) * 2048, -7).astype(np.int64)
    burst_len = np.where(used, rng.integers(1, 64, (n, slots)) * 2048, -7).astype(np.int32)
    flags = np.where(used, rng.choice([0, 0, 0, 1, 2, 3], (n, slots)), 0x7fff).astype(np.int32)
    nbytes = np.where(used, np.where(used, tap_len, 0) + rng.integers(0, 1 << 16, (n, slots)), 0x7fffffff)
    nbytes = nbytes.astype(np.int32).reshape(-1)
    if pattern == "wild":
        # values outside their ranges: the clamps decide, and the bytes behind a clamped tap_n are real bytes
        for c in np.nonzero(active)[0].tolist():
            kind = int(rng.integers(0, 5))
            if kind == 0:
                nc[c] = slots + int(rng.integers(1, 4))             # every slot counts, none beyond
                burst_start[c], burst_len[c], flags[c] = 2048 * c, 4096, 1
            elif kind == 1:
                nc[c] = -int(rng.integers(1, 4))                    # no slot counts
            elif kind == 2:
                tap_n[c] = cap + int(rng.integers(1, 1000))         # the whole row, no more
                tap_bytes[c] = rng.integers(0, marker, cap)
                if open_start[c] == 12345:
                    open_start[c] = 2048 * c
            elif kind == 3:
                tap_n[c] = -int(rng.integers(1, 1000))              # nothing
            elif nc[c] > 0:
                tap_len[c, 0] = -5 if rng.integers(0, 2) else cap + 7          # 0 bytes / all that tap_n leaves
    return nc, burst_start, burst_len, flags, nbytes, tap_bytes, tap_n, tap_len, open_start, open_nbytes


def partials(arrays):
    """``(channel, burst_start, offset, data, final)`` per segment straight from the arrays: what
    ``LiveResult.partials()`` lists."""
    return [(r[0], r[2], r[5], d, r[1] >= 0) for r, d in segments(*arrays)]
