"""The packed event list's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built
against tests/helpers (build_stub_live_lib.sh, loaded through tests/stub_lib.py), where "device" memory is host memory
and a launch records the kernel's name instead of running it.  On one copy of the library (``stub``: its last launch
and its number of launches): every argument check of afsk_live_events_layout and afsk_live_pack, and that a refused
call launches nothing.  On another copy (``logged``: its log of every launch): that a pack launches exactly its three
kernels, in order, by mangled name, behind the push entry's own launches, and that the push entry alone launches what
it launched before."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.live_push_cells import push_cell
from tests.stub_lib import last_kernel, launches

N, T, SLOTS, STRIDE = 600, 6144, 2, 24
PACK_KERNELS = ["_ZN4afsk22live_pack_total_kernelINS_14LiveEventsArgsEEEvT_",
                "_ZN4afsk21live_pack_scan_kernelENS_16LivePackScanArgsE",
                "_ZN4afsk24live_events_write_kernelENS_14LiveEventsArgsE"]
BAD = _native.E_INVALID_ARG
TABLES = (_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
          _native.LIVE_TAP_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES, _native.LIVE_EVENT_SIGNATURES)


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_events", TABLES)


@pytest.fixture(scope="module")
def logged(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_events_log", TABLES)


class Push:
    """Host buffers standing in for a push's device arrays and an events buffer."""

    def __init__(self, lib, n=N, slots=SLOTS, stride=STRIDE, max_events=40, max_bytes=500):
        self.n, self.slots, self.stride, self.max_events, self.max_bytes = n, slots, stride, max_events, max_bytes
        self.chunk = np.zeros((n, T), np.int16)
        self.n_closed = np.zeros(n, np.int32)
        self.start = np.zeros((n, slots), np.int64)
        self.rows = np.zeros((n * slots, max(stride, 1)), np.uint8)
        self.vec = [np.zeros(n * slots, np.int32) for _ in range(8)]      # len, flags, nbytes ... status, corrected
        total = C.c_int64()
        assert lib.afsk_live_events_layout(n, slots, max_events, max_bytes, C.byref(C.c_int64()), C.byref(C.c_int64()),
                                           C.byref(total)) == 0
        self.events = np.zeros(total.value // 16 + 1, np.dtype("V16"))   # (16-byte items: aligned enough after +0)
        self.ev_ptr = (self.events.ctypes.data + 15) & ~15

    def push_args(self, handle):
        p = lambda a: a.ctypes.data  # noqa: E731
        ln, flags, nbytes, nbits, ci, term, status, corrected = self.vec
        return [handle, p(self.chunk), T, T, 0, p(self.n_closed), p(self.start), p(ln), p(flags), p(self.rows),
                self.stride, p(nbytes), p(nbits), p(ci), p(term), p(status), p(corrected), None, 0, None]

    def pack_args(self, **change):
        p = lambda a: a.ctypes.data  # noqa: E731
        ln, flags, nbytes, nbits, ci, term, status, _ = self.vec
        a = dict(n_channels=self.n, slots=self.slots, n_closed=p(self.n_closed), burst_start=p(self.start),
                 burst_len=p(ln), flags=p(flags), out_bytes=p(self.rows), out_stride=self.stride, nbytes=p(nbytes),
                 nbits=p(nbits), clock_idx=p(ci), term_frame=p(term), status=p(status), events=self.ev_ptr,
                 max_events=self.max_events, max_bytes=self.max_bytes, hip_stream=None)
        assert set(change) <= set(a)
        a.update(change)
        return list(a.values())


def test_layout_argument_checks(stub):
    out = [C.c_int64() for _ in range(3)]
    refs = [C.byref(o) for o in out]
    for sizes in ((0, 2, 1, 1), (-1, 2, 1, 1), (4, 0, 1, 1), (4, -2, 1, 1), (1 << 16, 1 << 15, 1, 1),
                  (2 ** 31 - 1, 2, 1, 1), (4, 2, -1, 1), (4, 2, 1, -1), (4, 2, 1, 2 ** 31), (4, 2, 1, 2 ** 40)):
        assert stub.afsk_live_events_layout(*sizes, *refs) == BAD, sizes
    for missing in range(3):
        assert stub.afsk_live_events_layout(4, 2, 1, 1, *[None if i == missing else r for i, r in enumerate(refs)]) == BAD
    # the largest sizes that pass, and empty capacities
    assert stub.afsk_live_events_layout((1 << 16) - 1, 1 << 15, 2 ** 31 - 1, 2 ** 31 - 1, *refs) == 0
    assert stub.afsk_live_events_layout(1, 1, 0, 0, *refs) == 0
    assert [o.value for o in out] == [32, 32, 48]


def test_pack_argument_checks(stub):
    b = Push(stub)
    before = last_kernel(stub)[0]
    for change in (dict(n_channels=0), dict(n_channels=-3), dict(slots=0), dict(slots=-1),
                   dict(n_channels=1 << 16, slots=1 << 15), dict(max_events=-1), dict(max_bytes=-1),
                   dict(max_bytes=2 ** 31), dict(out_stride=-1), dict(events=b.ev_ptr + 4)):
        assert stub.afsk_live_pack(*b.pack_args(**change)) == BAD, change
    for ptr in ("n_closed", "burst_start", "burst_len", "flags", "out_bytes", "nbytes", "nbits", "clock_idx",
                "term_frame", "status", "events"):
        assert stub.afsk_live_pack(*b.pack_args(**{ptr: None})) == BAD, ptr
    assert last_kernel(stub)[0] == before                                  # nothing was launched
    # out_bytes may be NULL when there are no payload rows; empty capacities are fine
    assert stub.afsk_live_pack(*b.pack_args(out_bytes=None, out_stride=0)) == 0
    assert stub.afsk_live_pack(*b.pack_args(max_events=0, max_bytes=0)) == 0
    n, name, grid = last_kernel(stub)
    assert n == before + 6 and name == PACK_KERNELS[2] and grid == (N + 255) // 256


def test_a_pack_launches_its_three_kernels_in_order_and_nothing_else(logged):
    b = Push(logged)
    launches(logged)
    assert logged.afsk_live_pack(*b.pack_args()) == 0
    assert launches(logged) == PACK_KERNELS
    one = Push(logged, n=1, slots=3, stride=0, max_events=0, max_bytes=0)
    assert logged.afsk_live_pack(*one.pack_args(out_bytes=None)) == 0
    assert launches(logged) == PACK_KERNELS
    # the total and the write kernel are the event packer's own, the scan between them is neither packer's
    assert ["LiveEventsArgs" in k for k in PACK_KERNELS] == [True, False, True]
    assert not any("LiveSegmentsArgs" in k for k in PACK_KERNELS)


@pytest.mark.parametrize("kind", ["stored", "stream", "tap"])
def test_the_push_entry_then_the_pack_entry_launch_the_pushs_kernels_then_the_packs(logged, kind):
    """At the C level, the two calls ``LiveReceiver.push(events=)`` makes in its order, and the one call a push without
    ``events=`` makes (the stub library cannot hold torch tensors: the Python glue itself runs in the GPU tests, which
    compare its results and assert that a push without ``events=`` sets no ``events`` attribute)."""
    n = 6
    bf = np.ascontiguousarray([40, 160] * (n // 2), np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    thr = lambda v: np.full(n, v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    h = C.c_void_p()
    if kind == "stored":
        assert logged.afsk_live_create_thresholds(n, bf, thr(18000), thr(14000), 48000, T, C.byref(h)) == 0
    elif kind == "stream":
        assert logged.afsk_live_create_stream_thresholds(n, bf, thr(18000), thr(14000), STRIDE, T, C.byref(h)) == 0
    else:
        assert logged.afsk_live_create_stream_tap(n, bf, thr(18000), thr(14000), STRIDE, T, C.byref(h)) == 0
    b = Push(logged, n=n)
    launches(logged)
    assert logged.afsk_live_push(*b.push_args(h)) == 0
    alone = launches(logged)
    sink = "stored" if kind == "stored" else "stream"
    assert push_cell(alone[0]) == (sink, False, False)
    # (a stored push with out_corrected zeroes that array ahead of its demod launch: clear_corrected)
    rest = ["clear" if "clear_i32_kernel" in k else k for k in alone[1:]]
    assert rest == (["clear", "demod"] if kind == "stored" else [])
    # push, then pack: the push's launches followed by the pack's
    assert logged.afsk_live_push(*b.push_args(h)) == 0
    assert logged.afsk_live_pack(*b.pack_args()) == 0
    assert launches(logged) == alone + PACK_KERNELS
    # and a push alone still launches what it launched
    assert logged.afsk_live_push(*b.push_args(h)) == 0
    assert launches(logged) == alone
    assert logged.afsk_live_destroy(h) == 0
