"""Host side of the packed segment list (no GPU): the C-ABI declarations and their signature table, the layout entry
against its documented arithmetic, the record dtype against the header's struct, the argument checks that need no
device, ``LiveSegments`` parsing numpy-backed buffers built by the model (tests/live_segments_model.py) -- with enough
room, with fewer records than segments, and with the data cut at ``max_bytes`` -- and ``PayloadAssembler.feed`` taking
segment lists in place of results over a sequence of pushes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from afskmodem_amd import _native, batch, live
from tests import live_segments_model as M
from tests.test_live_ragged_host import declared_args, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("afsk_live_segments_layout", "afsk_live_pack_tap")
SPAN = 256


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_SEGMENT_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_SEGMENT_SIGNATURES[name]
        want = declared_args(hdr, name)
        # (a pointer is bound as void * or, the layout's host outputs, as a typed pointer)
        assert res is C.c_int and len(args) == len(want), name
        assert all(a is w or (w is C.c_void_p and issubclass(a, C._Pointer)) for a, w in zip(args, want)), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_pack(")
        assert getattr(C.CDLL(_native.LIB_PATH), name) is not None
        assert getattr(_native.lib(), name).argtypes == args
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_SEGMENT_SIGNATURES"]
    assert len(others) >= 11 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_LIVE_EVENTS_SPAN (\d+)", hdr).group(1)) == SPAN
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_segment_dtype_matches_the_header_struct(tmp_path):
    assert live.SEGMENT_DTYPE.itemsize == 32 and live.SEGMENT_DTYPE == M.SEGMENT
    assert live.EVENTS_HEADER_DTYPE == M.HEADER
    names = live.SEGMENT_DTYPE.names
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "afsk_amd.h"\nint main(void) {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(afsk_live_segment, {f}));\n' for f in names)
                   + '  printf("sizeof %zu\\n", sizeof(afsk_live_segment));\n  return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == 32
    assert list(got) == list(names)                                                  # the fields, in order
    assert {f: int(v) for f, v in got.items()} == {f: live.SEGMENT_DTYPE.fields[f][1] for f in names}
    body = re.search(r"typedef struct afsk_live_segment \{(.*?)\} afsk_live_segment;", header(), flags=re.S).group(1)
    members = [m.split() for m in body.replace("\n", " ").split(";") if m.strip()]
    assert [(t, f) for t, f in members] == [("int64_t" if f == "burst_start" else "int32_t", f) for f in names]


def test_segments_layout_follows_its_documented_arithmetic():
    for n, slots, ms, mb in ((1, 1, 0, 0), (1, 1, 1, 1), (255, 2, 7, 15), (256, 2, 7, 16), (257, 2, 7, 17),
                             (257, 3, 257 * 4, 257 * 19), (65536, 2, 65536 * 3, 65536 * 19),
                             (1 << 20, 2047, 5, 2 ** 31 - 1), (2 ** 31 - 1, 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        ro, do, total = live.segments_layout(n, slots, ms, mb)
        assert ro == 32 and do == 32 + 32 * ms
        assert total == (do + mb + 15) // 16 * 16 + 16 * ((n + SPAN - 1) // SPAN)
    assert live.segments_layout(1, 1, 0, 0) == (32, 32, 48)
    assert live.segments_layout(257, 2, 4, 8)[2] > live.segments_layout(256, 2, 4, 8)[2]


def test_both_entries_refuse_bad_sizes_and_null_pointers_without_a_device():
    lib = _native.lib()
    out = [C.c_int64() for _ in range(3)]
    refs = [C.byref(o) for o in out]
    bad = _native.E_INVALID_ARG
    # what afsk_live_events_layout refuses, with its codes
    for sizes in ((0, 1, 1, 1), (1, 0, 1, 1), (1 << 16, 1 << 15, 1, 1), (4, 2, -1, 1), (4, 2, 1, -1), (4, 2, 1, 2 ** 31)):
        assert lib.afsk_live_events_layout(*sizes, *refs) == bad, sizes
        assert lib.afsk_live_segments_layout(*sizes, *refs) == bad, sizes
        with pytest.raises(_native.AfskNativeError):
            live.segments_layout(*sizes)
    for missing in range(3):
        assert lib.afsk_live_segments_layout(4, 2, 1, 1, *[None if i == missing else r for i, r in enumerate(refs)]) == bad
    assert lib.afsk_live_segments_layout((1 << 16) - 1, 1 << 15, 1, 2 ** 31 - 1, *refs) == 0
    # afsk_live_pack_tap checks its arguments before it looks for a device
    a = np.zeros(64, np.int64)
    p = a.ctypes.data
    arrays = [p] * 10
    assert lib.afsk_live_pack_tap(0, 1, 4, *arrays, p, 1, 1, None) == bad
    assert lib.afsk_live_pack_tap(1, 1, 0, *arrays, p, 1, 1, None) == bad
    assert "tap_cap" in _native.last_error()
    assert lib.afsk_live_pack_tap(1, 1, 4, None, *arrays[1:], p, 1, 1, None) == bad
    assert "null pointer" in _native.last_error()
    assert lib.afsk_live_pack_tap(1, 1, 4, *arrays, p + 8, 1, 1, None) == bad
    if _native.device_count() <= 0:
        assert lib.afsk_live_pack_tap(1, 1, 4, *arrays, p, 1, 1, None) == _native.E_NO_DEVICE


# --------------------------------------------------------------------------- LiveSegments on numpy-backed buffers

def host_result(arrays):
    nc, start, length, flags, nbytes, tap_bytes, tap_n, tap_len, open_start, open_nbytes = arrays
    z = np.zeros(nbytes.size, np.int32)
    return live.LiveResult(nc, start, length, flags, batch.HostDemodResult(np.zeros((nbytes.size, 0), np.uint8), nbytes,
                                                                           z, z, z, z),
                           live.LiveTap(tap_bytes, tap_n, tap_len, open_start, open_nbytes))


def host_segments(arrays, result, max_segments, max_bytes):
    h, recs, data = M.pack(arrays, max_segments, max_bytes)
    sg = live.LiveSegments(M.buffer(h, recs, data, max_segments, max_bytes), max_segments, max_bytes, result=result)
    return sg, h, recs, data


@pytest.mark.parametrize("pattern", ["nothing", "open_only", "all", "span_last", "random", "orphan"])
def test_live_segments_parses_a_buffer_with_room_for_everything(pattern):
    arrays = M.random_tap(np.random.default_rng(3), 70, 3, 19, pattern, span=16)
    want = host_result(arrays).partials()
    assert want == M.partials(arrays) and (len(want) > 0) == (pattern != "nothing")
    count, nb = len(want), sum(len(w[3]) for w in want)
    sg, h, recs, data = host_segments(arrays, None, count + 2, nb + 3)       # (no result: nothing may be missing)
    assert (sg.count, sg.stored, sg.overflowed) == (count, count, False)
    assert sg.partials() == want
    assert sg.copied_bytes == 32 + 32 * count + nb                             # header, records, data: no more
    got = sg.records()
    assert got.dtype == live.SEGMENT_DTYPE and got.tobytes() == recs.tobytes()
    if pattern == "orphan":
        assert nb < int(np.clip(arrays[6], 0, 19).sum())                       # bytes nobody owns stayed behind
    if pattern in ("all", "random"):
        assert any(w[4] and not w[3] for w in want) or pattern == "all"
        assert any(w[4] for w in want) and any(not w[4] for w in want)


def test_live_segments_falls_back_to_the_result_past_max_segments():
    arrays = M.random_tap(np.random.default_rng(5), 70, 3, 19, "all")
    result = host_result(arrays)
    want = result.partials()
    sg, h, _, _ = host_segments(arrays, result, len(want) - 4, 70 * 19)
    assert (sg.count, sg.stored, sg.overflowed) == (len(want), len(want) - 4, True)
    assert sg.records().size == len(want) - 4
    assert sg.partials() == want
    tap = result.tap
    whole = sum(a.nbytes for a in (arrays[0], arrays[1], arrays[4], tap.bytes, tap.n, tap.len, tap.open_start,
                                   tap.open_nbytes))
    assert sg.copied_bytes == 32 + whole                                       # the header, then what partials() copies
    sg.result = None
    with pytest.raises(ValueError):
        sg.partials()


def test_live_segments_falls_back_to_the_result_for_unwritten_data():
    arrays = M.random_tap(np.random.default_rng(7), 70, 3, 19, "random")
    result = host_result(arrays)
    want = result.partials()
    total = sum(len(w[3]) for w in want)
    sg, h, recs, data = host_segments(arrays, result, len(want), total // 2)
    assert int(h["stored_bytes"][0]) == len(data) <= total // 2 < int(h["n_bytes"][0]) == total
    assert sg.overflowed and sg.stored == sg.count == len(want)
    assert sg.partials() == want
    sg.result = None
    with pytest.raises(ValueError):
        sg.partials()
    with pytest.raises(ValueError):
        live.PayloadAssembler().feed(sg)


# ------------------------------------------------------------------------------- PayloadAssembler.feed(LiveSegments)

N, SLOTS, CAP = 6, 2, 12
OPEN_END, OVERFLOW = _native.LIVE_OPEN_END, _native.LIVE_OVERFLOW


def push_arrays(finals=(), opens=(), recording=()):
    """One push's arrays.  ``finals``: (channel, start, burst_len, flags, nbytes, data) per reported burst, in order;
    ``opens``: (channel, start, nbytes so far, data) per channel whose open burst decoded bytes; ``recording``:
    (channel, start) per channel whose burst is open and decoded nothing in this push."""
    nc = np.zeros(N, np.int32)
    start = np.full((N, SLOTS), -7, np.int64)
    length, flags = np.full((N, SLOTS), -7, np.int32), np.full((N, SLOTS), 0x7fff, np.int32)
    nbytes = np.full(N * SLOTS, 0x7fffffff, np.int32)
    tap_bytes, tap_n, tap_len = np.full((N, CAP), 0xEE, np.uint8), np.zeros(N, np.int32), np.zeros((N, SLOTS), np.int32)
    open_start, open_nbytes = np.full(N, -1, np.int64), np.zeros(N, np.int32)

    def put(c, data):
        tap_bytes[c, tap_n[c]: tap_n[c] + len(data)] = np.frombuffer(data, np.uint8)
        tap_n[c] += len(data)

    for c, s, ln, fl, nb, data in finals:
        k = int(nc[c])
        start[c, k], length[c, k], flags[c, k], nbytes[c * SLOTS + k], tap_len[c, k] = s, ln, fl, nb, len(data)
        nc[c] = k + 1
        put(c, data)
    for c, s, nb, data in opens:
        open_start[c], open_nbytes[c] = s, nb
        put(c, data)
    for c, s in recording:
        open_start[c] = s
    return nc, start, length, flags, nbytes, tap_bytes, tap_n, tap_len, open_start, open_nbytes


SEQUENCE = [
    # bursts open on channels 0 ... 3
    push_arrays(opens=[(0, 2048, 2, b"ab"), (1, 4096, 3, b"xyz"), (2, 0, 1, b"q"), (3, 2048, 9, b"too long ")]),
    # 0 closes with no new bytes; 1 closes with bytes and its next burst opens; 2 records on without bytes; 3 closes
    # overflowed, which withdraws what it sent
    push_arrays(finals=[(0, 2048, 8192, 0, 2, b""), (1, 4096, 6144, 0, 5, b"12"), (3, 2048, 1 << 20, OVERFLOW, 0, b"")],
                opens=[(1, 12288, 1, b"N")], recording=[(2, 0)]),
    # channel 2 was reset in mid-burst: nothing is open there any more; two bursts of channel 4 in one push
    push_arrays(finals=[(4, 2048, 2048, 0, 1, b"A"), (4, 6144, 4096, 0, 2, b"BC")], opens=[(1, 12288, 2, b"M")]),
    # channel 2 starts over; channel 1 was reset too and records a new burst that already has bytes
    push_arrays(opens=[(2, 8192, 1, b"r"), (1, 20480, 4, b"new!")]),
    # a push in which nothing happened
    push_arrays(recording=[(2, 8192), (1, 20480)]),
    # the flush: what was open is reported open-ended
    push_arrays(finals=[(2, 8192, 4096, OPEN_END, 2, b"s"), (1, 20480, 2048, OPEN_END, 5, b"?")]),
]
WANT = [[], [(0, 2048, 8192, b"ab"), (1, 4096, 6144, b"xyz12"), (3, 2048, 1 << 20, b"")],
        [(4, 2048, 2048, b"A"), (4, 6144, 4096, b"BC")], [], [], [(1, 20480, 2048, b"new!?"), (2, 8192, 4096, b"rs")]]
PENDING = [{0: (2048, b"ab"), 1: (4096, b"xyz"), 2: (0, b"q"), 3: (2048, b"too long ")},
           {1: (12288, b"N"), 2: (0, b"q")}, {1: (12288, b"NM")}, {1: (20480, b"new!"), 2: (8192, b"r")},
           {1: (20480, b"new!"), 2: (8192, b"r")}, {}]
# held bursts whose channel had no open segment in the push (open_start is gathered there): channel 2 records on without
# bytes in push 1, is found dropped in push 2; channels 1 and 2 record on without bytes in push 4
GATHERED = [0, 1, 1, 0, 2, 0]


class OpenStartOnly:
    """A result of which only ``tap.open_start`` may be touched."""

    def __init__(self, open_start):
        self.tap = type("Tap", (), {"open_start": open_start})()


@pytest.mark.parametrize("room", ["all", "records_short", "bytes_short"])
def test_the_assembler_takes_segments_in_place_of_results(room):
    by_result, by_segments = live.PayloadAssembler(), live.PayloadAssembler()
    for p, arrays in enumerate(SEQUENCE):
        result = host_result(arrays)
        want = by_result.feed(result)
        assert want == WANT[p] and by_result.pending() == PENDING[p], p
        count, nb = len(M.segments(*arrays)), int(np.sum(arrays[6]))
        if room == "all":
            # the packed list alone: of the result, only open_start is there to be read, and only where a burst is held
            sg, _, _, _ = host_segments(arrays, OpenStartOnly(arrays[8]), count, nb)
        else:
            sg, _, _, _ = host_segments(arrays, result, *((max(count - 1, 0), nb) if room == "records_short"
                                                          else (count, max(nb - 1, 0))))
            assert sg.overflowed == (count > 0 if room == "records_short" else nb > 0)
        assert by_segments.feed(sg) == want, p
        assert by_segments.pending() == PENDING[p], p
        if room == "all":
            assert sg.copied_bytes == 32 + 32 * count + nb + 8 * GATHERED[p], p


def test_results_and_segments_may_alternate():
    mixed = live.PayloadAssembler(string=True)
    text = lambda rows: [r[:3] + (r[3].decode() if r[3] else b"",) for r in rows]  # noqa: E731
    for p, arrays in enumerate(SEQUENCE):
        result = host_result(arrays)
        x = result if p % 2 else host_segments(arrays, result, 3 * N, N * CAP)[0]
        assert mixed.feed(x) == text(WANT[p]), p
        assert mixed.pending() == PENDING[p], p


# ------------------------------------------------------------------------------------- the model's two forms agree

def same_pack(arrays, max_segments, max_bytes, tag):
    """``pack_fast`` -- over the tap rows, and over their width alone -- is ``pack``: header, records, data."""
    h, recs, data = M.pack(arrays, max_segments, max_bytes)
    cap = arrays[5].shape[1]
    for rows in (arrays[5], cap):
        fh, frecs, copies = M.pack_fast((*arrays[:5], rows, *arrays[6:]), max_segments, max_bytes)
        assert fh.dtype == M.HEADER and fh.tobytes() == h.tobytes(), (tag, fh, h)
        assert frecs.dtype == M.SEGMENT and frecs.tobytes() == recs.tobytes(), tag
        for f in M.SEGMENT.names:
            assert np.array_equal(frecs[f], recs[f]), (tag, f)
        assert copies.shape == (recs.size, 4) and copies.dtype == np.int64
        assert M.gather(arrays[5], copies) == data, tag
        written = copies[:, 3] >= 0
        assert np.array_equal(copies[:, 0], recs["channel"]) and (copies[~written, 2] == 0).all()
        assert np.array_equal(copies[written, 2], recs["length"][written])
        assert ((copies[:, 1] >= 0) & (copies[:, 1] + recs["length"] <= cap)).all()
    return h[0], recs


@pytest.mark.parametrize("n", [1, 255, 256, 257, 775])
@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_pack_fast_is_pack(n, pattern):
    rng = np.random.default_rng(2000 + n)
    for slots in (1, 2, 3):
        for cap in (1, 19, 183):
            arrays = M.random_tap(rng, n, slots, cap, pattern)
            same_pack(arrays, n * (slots + 1), n * cap, (slots, cap, "room"))
            same_pack(arrays, n, 40, (slots, cap, "short"))


def test_pack_fast_is_pack_at_every_capacity_edge():
    """The capacities of the GPU module's test_capacities_bound_what_is_written."""
    rng = np.random.default_rng(9)
    n, slots, cap = 2 * SPAN + 150, 2, 19
    arrays = M.random_tap(rng, n, slots, cap, "random")
    segs = M.segments(*arrays)
    count, nb = len(segs), sum(len(d) for _, d in segs)
    assert count > 100 and nb > 400
    for max_segments in (count - 1, count, count + 1):
        for max_bytes in (nb - 1, nb, nb + 1):
            same_pack(arrays, max_segments, max_bytes, (max_segments, max_bytes))
    off = 0
    for i, (r, d) in enumerate(segs):                       # a data part that ends inside ONE channel's run
        nxt = segs[i + 1] if i + 1 < count else None
        if i > count // 2 and r[1] >= 0 and len(d) > 0 and nxt and nxt[0][0] == r[0] and len(nxt[1]) > 1:
            cut = off + len(d) + 1
            break
        off += len(d)
    else:
        raise AssertionError("no channel with two segments that hold bytes")
    h, _ = same_pack(arrays, count, cut, "straddle")
    assert h["stored_bytes"] == cut - 1 and h["stored"] == count
    h, recs = same_pack(arrays, i + 1, nb, "records straddle")
    assert h["stored_bytes"] == cut - 1 and recs["channel"][-1] == segs[i + 1][0][0]
    h, _ = same_pack(arrays, 0, 0, "nothing")
    assert (h["count"], h["stored"], h["n_bytes"], h["stored_bytes"]) == (count, 0, nb, 0)
