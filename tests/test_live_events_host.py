"""Host side of the packed event list (no GPU): the C-ABI declarations and their signature table, the layout entry
against its documented arithmetic, the record dtype against the header's struct, the argument checks that need no
device, and ``LiveEvents`` parsing numpy-backed buffers built by the model (tests/live_events_model.py) -- with enough
room, with fewer records than bursts, and with fewer payload bytes than the bursts keep."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from afskmodem_amd import _native, batch, live
from tests import live_events_model as M
from tests.test_live_ragged_host import declared_args, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("afsk_live_events_layout", "afsk_live_pack")
SPAN = 256


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_EVENT_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_EVENT_SIGNATURES[name]
        want = declared_args(hdr, name)
        # (a pointer is bound as void * or, the layout's host outputs, as a typed pointer)
        assert res is C.c_int and len(args) == len(want), name
        assert all(a is w or (w is C.c_void_p and issubclass(a, C._Pointer)) for a, w in zip(args, want)), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_push_ragged(")
        assert getattr(C.CDLL(_native.LIB_PATH), name) is not None
        assert getattr(_native.lib(), name).argtypes == args
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_EVENT_SIGNATURES"]
    assert all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_LIVE_EVENTS_SPAN (\d+)", hdr).group(1)) == SPAN
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_event_dtype_matches_the_header_struct(tmp_path):
    assert live.EVENT_DTYPE.itemsize == 48 and live.EVENT_DTYPE == M.EVENT
    assert live.EVENTS_HEADER_DTYPE.itemsize == 32 and live.EVENTS_HEADER_DTYPE == M.HEADER
    names = live.EVENT_DTYPE.names
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "afsk_amd.h"\nint main(void) {\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(afsk_live_event, {f}));\n' for f in names)
                   + '  printf("sizeof %zu\\n", sizeof(afsk_live_event));\n  return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == 48
    assert list(got) == list(names)                                                  # the fields, in order
    assert {f: int(v) for f, v in got.items()} == {f: live.EVENT_DTYPE.fields[f][1] for f in names}
    # the struct's member types, from the header's text
    body = re.search(r"typedef struct afsk_live_event \{(.*?)\} afsk_live_event;", header(), flags=re.S).group(1)
    members = [m.split() for m in body.replace("\n", " ").split(";") if m.strip()]
    assert [(t, f) for t, f in members] == [("int64_t" if f == "burst_start" else "int32_t", f) for f in names]


def test_events_layout_follows_its_documented_arithmetic():
    for n, slots, me, mb in ((1, 1, 0, 0), (1, 1, 1, 1), (255, 2, 7, 15), (256, 2, 7, 16), (257, 2, 7, 17),
                             (257, 3, 771, 771 * 384), (65536, 2, 131072, 131072 * 172),
                             (1 << 20, 2047, 5, 2 ** 31 - 1), (2 ** 31 - 1, 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        ro, po, total = live.events_layout(n, slots, me, mb)
        assert ro == 32 and po == 32 + 48 * me
        assert ro % 16 == 0 and po % 16 == 0 and total % 16 == 0
        assert total == (po + mb + 15) // 16 * 16 + 16 * ((n + SPAN - 1) // SPAN)
    # total_bytes grows monotonically in every capacity
    for me in range(1, 4):
        for mb in range(1, 40):
            total = live.events_layout(300, 2, me, mb)[2]
            assert total >= live.events_layout(300, 2, me, mb - 1)[2]
            assert total > live.events_layout(300, 2, me - 1, mb)[2]
            assert total > live.events_layout(300, 2, me, mb - 16)[2] if mb >= 16 else True
    assert live.events_layout(257, 2, 4, 8)[2] > live.events_layout(256, 2, 4, 8)[2]


def test_both_entries_refuse_bad_sizes_and_null_pointers_without_a_device():
    lib = _native.lib()
    out = [C.c_int64() for _ in range(3)]
    refs = [C.byref(o) for o in out]
    bad = _native.E_INVALID_ARG
    for sizes in ((0, 1, 1, 1), (1, 0, 1, 1), (1 << 16, 1 << 15, 1, 1), (4, 2, -1, 1), (4, 2, 1, -1), (4, 2, 1, 2 ** 31)):
        assert lib.afsk_live_events_layout(*sizes, *refs) == bad, sizes
        with pytest.raises(_native.AfskNativeError):
            live.events_layout(*sizes)
    for missing in range(3):
        assert lib.afsk_live_events_layout(4, 2, 1, 1, *[None if i == missing else r for i, r in enumerate(refs)]) == bad
    assert lib.afsk_live_events_layout((1 << 16) - 1, 1 << 15, 1, 2 ** 31 - 1, *refs) == 0
    # afsk_live_pack checks its arguments before it looks for a device
    a = np.zeros(64, np.int64)
    p = a.ctypes.data
    assert lib.afsk_live_pack(0, 1, p, p, p, p, p, 4, p, p, p, p, p, p, 1, 1, None) == bad
    assert lib.afsk_live_pack(1, 1, None, p, p, p, p, 4, p, p, p, p, p, p, 1, 1, None) == bad
    assert "null pointer" in _native.last_error()
    if _native.device_count() <= 0:
        assert lib.afsk_live_pack(1, 1, p, p, p, p, p, 4, p, p, p, p, p, p, 1, 1, None) == _native.E_NO_DEVICE


# ----------------------------------------------------------------------------- LiveEvents on numpy-backed buffers

def host_push(seed, n=70, slots=3, stride=12, pattern="sparse"):
    rng = np.random.default_rng(seed)
    nc, start, length, flags, rows, demod = M.random_push(rng, n, slots, stride, pattern)
    result = live.LiveResult(nc, start, length, flags,
                             batch.HostDemodResult(rows, *(demod[f] for f in ("nbytes", "nbits", "clock_idx",
                                                                              "term_frame", "status"))))
    return (nc, start, length, flags, rows, demod), result


def host_events(arrays, result, max_events, max_bytes):
    h, recs, pay = M.pack(*arrays, max_events, max_bytes)
    return live.LiveEvents(M.buffer(h, recs, pay, max_events, max_bytes), max_events, max_bytes, result=result), h, recs


@pytest.mark.parametrize("pattern", ["sparse", "full", "zero", "first", "last"])
def test_live_events_parses_a_buffer_with_room_for_everything(pattern):
    arrays, result = host_push(3, pattern=pattern)
    want = M.slot_bursts(*arrays)
    count = int(arrays[0].sum())
    assert len(want) == count and (count > 0) == (pattern != "zero")
    ev, h, recs = host_events(arrays, None, count + 2, count * 12 + 3)       # (no result: nothing may be missing)
    assert (ev.count, ev.stored, ev.overflowed) == (count, count, False)
    assert ev.bursts() == want
    assert ev.copied_bytes == 32 + 48 * count + int(h["stored_bytes"][0])       # header, records, payload: no more
    got = ev.records()
    assert got.dtype == live.EVENT_DTYPE and got.tobytes() == recs.tobytes()
    assert [ev.payload(i) for i in range(count)] == [w[3] for w in want]
    if pattern == "full":
        assert any(r["flags"] & M.OVERFLOW for r in recs) and any(r["nbytes"] > 12 for r in recs)


def test_live_events_falls_back_to_the_result_past_max_events():
    arrays, result = host_push(5, pattern="full")
    want = M.slot_bursts(*arrays)
    ev, h, _ = host_events(arrays, result, len(want) - 4, len(want) * 12)
    assert (ev.count, ev.stored, ev.overflowed) == (len(want), len(want) - 4, True)
    assert ev.records().size == len(want) - 4
    assert ev.bursts() == want
    ev.result = None
    with pytest.raises(ValueError):
        ev.bursts()


def test_live_events_falls_back_to_the_result_for_unwritten_payloads():
    arrays, result = host_push(7, pattern="full")
    want = M.slot_bursts(*arrays)
    total = sum(len(w[3]) for w in want)
    ev, h, recs = host_events(arrays, result, len(want), total // 2)
    minus = np.nonzero(recs["payload_offset"] == -1)[0]
    assert 0 < minus.size < len(want) and int(h["stored_bytes"][0]) <= total // 2 < int(h["n_bytes"][0]) == total
    assert ev.overflowed and ev.stored == ev.count == len(want)
    assert ev.bursts() == want
    assert [ev.payload(i) for i in range(len(want))] == [w[3] for w in want]
    ev.result = None
    with pytest.raises(ValueError):
        ev.bursts()


def test_live_events_returns_text_like_bursts():
    nc = np.array([0, 2], np.int32)
    start = np.array([[0, 0], [2048, 8192]], np.int64)
    length = np.array([[0, 0], [4096, 2048]], np.int32)
    flags = np.zeros((2, 2), np.int32)
    rows = np.zeros((4, 8), np.uint8)
    rows[2, :5] = np.frombuffer(b"hello", np.uint8)
    demod = {f: np.zeros(4, np.int32) for f in M.FIELDS}
    demod["nbytes"][2] = 5
    h, recs, pay = M.pack(nc, start, length, flags, rows, demod, 4, 32)
    ev = live.LiveEvents(M.buffer(h, recs, pay, 4, 32), 4, 32)
    assert ev.bursts(string=True) == [(1, 2048, 4096, "hello"), (1, 8192, 2048, b"")]
    assert ev.bursts() == [(1, 2048, 4096, b"hello"), (1, 8192, 2048, b"")]


# ------------------------------------------------------------------------------------- the model's two forms agree

def same_pack(arrays, max_events, max_bytes, tag):
    """``pack_fast`` -- over the rows, and over their stride alone -- is ``pack``: header, records, payload."""
    h, recs, pay = M.pack(*arrays, max_events, max_bytes)
    stride = arrays[4].shape[1]
    for rows in (arrays[4], stride):
        fh, frecs, copies = M.pack_fast(*arrays[:4], rows, arrays[5], max_events, max_bytes)
        assert fh.dtype == M.HEADER and fh.tobytes() == h.tobytes(), (tag, fh, h)
        assert frecs.dtype == M.EVENT and frecs.tobytes() == recs.tobytes(), tag
        for f in M.EVENT.names:
            assert np.array_equal(frecs[f], recs[f]), (tag, f)
        assert copies.shape == (recs.size, 4) and copies.dtype == np.int64
        assert M.gather(arrays[4], copies) == pay, tag
        written = copies[:, 2] > 0
        assert np.array_equal(copies[written, 3], recs["payload_offset"][written])
        assert np.array_equal(copies[:, 0], recs["channel"].astype(np.int64) * arrays[2].shape[1] + recs["slot"])
        assert (copies[:, 1] == 0).all() and (copies[~written, 2] == 0).all()
    return h[0], recs


@pytest.mark.parametrize("n", [1, 255, 256, 257, 775])
@pytest.mark.parametrize("pattern", ["zero", "full", "sparse", "last", "first", "wild"])
def test_pack_fast_is_pack(n, pattern):
    rng = np.random.default_rng(1000 + n)
    for slots in (1, 2, 3):
        for stride in (0, 12, 172):
            arrays = M.random_push(rng, n, slots, stride, pattern)
            same_pack(arrays, n * slots, n * slots * stride, (slots, stride, "room"))
            same_pack(arrays, n, 40, (slots, stride, "short"))


def test_the_wild_pattern_meets_both_ends_of_the_clamp():
    rng = np.random.default_rng(4)
    n, slots, stride = 775, 2, 12
    arrays = M.random_push(rng, n, slots, stride, "wild")
    nc = arrays[0]
    below, above = nc < 0, nc > slots
    assert below.sum() > 3 and above.sum() > 3 and ((nc > 0) & ~above).sum() > 3
    assert set(nc[below].tolist()) <= {-3, -2, -1} and set(nc[above].tolist()) <= {slots + 1, slots + 2, slots + 3}
    h, recs = same_pack(arrays, n * slots, n * slots * stride, "wild")
    assert h["count"] == np.clip(nc, 0, slots).sum() < np.abs(nc).sum()
    assert not set(recs["channel"].tolist()) & set(np.nonzero(below)[0].tolist())
    for c in np.nonzero(above)[0].tolist():                                     # every slot, and none beyond
        assert recs["slot"][recs["channel"] == c].tolist() == list(range(slots))
    assert (recs["burst_len"] > 0).all() and (recs["flags"] <= 3).all()        # (only slots that hold a burst)
    assert [b[0] for b in M.slot_bursts(*arrays)] == recs["channel"].tolist()


def test_pack_fast_is_pack_at_every_capacity_edge():
    """The capacities of the GPU module's test_capacities_bound_what_is_written."""
    rng = np.random.default_rng(9)
    n, slots, stride = 2 * SPAN + 150, 2, 172
    arrays = M.random_push(rng, n, slots, stride, "sparse")
    full, all_recs, _ = M.pack(*arrays, n * slots, n * slots * stride)
    count, kept = int(full["count"][0]), int(full["n_bytes"][0])
    assert count > 8 and kept > 400
    for max_events in (count - 1, count, count + 1):
        for max_bytes in (kept - 1, kept, kept + 1):
            same_pack(arrays, max_events, max_bytes, (max_events, max_bytes))
    h, recs = same_pack(arrays, count, int(all_recs["payload_offset"][count // 2]), "cut")
    assert (recs["payload_offset"] == -1).any() and (recs["payload_offset"] >= 0).any()
    h, recs = same_pack(arrays, 0, 0, "nothing")
    assert (h["count"], h["stored"], h["n_bytes"], h["stored_bytes"]) == (count, 0, kept, 0)
