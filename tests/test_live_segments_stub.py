"""The packed segment list's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built
against tests/helpers (build_stub_live_lib.sh, loaded through tests/stub_lib.py), where "device" memory is host memory
and a launch records the kernel's name instead of running it.  On one copy of the library (``stub``: its last launch
and its number of launches): every argument check of afsk_live_segments_layout and afsk_live_pack_tap, and that a
refused call launches nothing.  On another copy (``logged``: its log of every launch): that a pack launches exactly its
three kernels, in order, by mangled name, behind the tapped push's own launches, and that the push alone launches what
it launched before."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.live_push_cells import push_cell
from tests.stub_lib import last_kernel, launches
from tests.test_live_events_stub import PACK_KERNELS as EVENT_KERNELS
from tests.test_live_events_stub import TABLES as EVENT_TABLES
from tests.test_live_events_stub import Push

N, T, SLOTS, STRIDE, CAP = 600, 6144, 2, 24, 19
PACK_KERNELS = ["_ZN4afsk22live_pack_total_kernelINS_16LiveSegmentsArgsEEEvT_",
                "_ZN4afsk21live_pack_scan_kernelENS_16LivePackScanArgsE",
                "_ZN4afsk26live_segments_write_kernelENS_16LiveSegmentsArgsE"]
BAD = _native.E_INVALID_ARG


TABLES = EVENT_TABLES + (_native.LIVE_SEGMENT_SIGNATURES,)


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_segments", TABLES)


@pytest.fixture(scope="module")
def logged(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_segments_log", TABLES)


class TapPush(Push):
    """``Push`` with the five tap arrays and a segments buffer."""

    def __init__(self, lib, n=N, slots=SLOTS, cap=CAP, max_segments=40, max_bytes=500):
        super().__init__(lib, n=n, slots=slots)
        self.cap, self.max_segments, self.seg_bytes = cap, max_segments, max_bytes
        self.tap_bytes = np.zeros((n, cap), np.uint8)
        self.tap_n, self.tap_len = np.zeros(n, np.int32), np.zeros((n, slots), np.int32)
        self.open_start, self.open_nbytes = np.full(n, -1, np.int64), np.zeros(n, np.int32)
        total = C.c_int64()
        assert lib.afsk_live_segments_layout(n, slots, max_segments, max_bytes, C.byref(C.c_int64()),
                                             C.byref(C.c_int64()), C.byref(total)) == 0
        self.segments = np.zeros(total.value // 16 + 1, np.dtype("V16"))
        self.sg_ptr = (self.segments.ctypes.data + 15) & ~15

    def tap_ptrs(self):
        return [a.ctypes.data for a in (self.tap_bytes, self.tap_n, self.tap_len, self.open_start, self.open_nbytes)]

    def tapped_push_args(self, handle):
        return self.push_args(handle)[:-1] + self.tap_ptrs() + [None]

    def seg_args(self, **change):
        p = lambda a: a.ctypes.data  # noqa: E731
        ln, flags, nbytes = self.vec[:3]
        tb, tn, tl, os_, on = self.tap_ptrs()
        a = dict(n_channels=self.n, slots=self.slots, tap_cap=self.cap, n_closed=p(self.n_closed),
                 burst_start=p(self.start), burst_len=p(ln), flags=p(flags), nbytes=p(nbytes), tap_bytes=tb, tap_n=tn,
                 tap_len=tl, open_start=os_, open_nbytes=on, segments=self.sg_ptr, max_segments=self.max_segments,
                 max_bytes=self.seg_bytes, hip_stream=None)
        assert set(change) <= set(a)
        a.update(change)
        return list(a.values())


def test_layout_argument_checks(stub):
    out = [C.c_int64() for _ in range(3)]
    refs = [C.byref(o) for o in out]
    for sizes in ((0, 2, 1, 1), (-1, 2, 1, 1), (4, 0, 1, 1), (4, -2, 1, 1), (1 << 16, 1 << 15, 1, 1),
                  (2 ** 31 - 1, 2, 1, 1), (4, 2, -1, 1), (4, 2, 1, -1), (4, 2, 1, 2 ** 31), (4, 2, 1, 2 ** 40)):
        assert stub.afsk_live_segments_layout(*sizes, *refs) == BAD, sizes
        assert stub.afsk_live_events_layout(*sizes, *refs) == BAD, sizes           # the same refusals
    for missing in range(3):
        assert stub.afsk_live_segments_layout(4, 2, 1, 1, *[None if i == missing else r for i, r in enumerate(refs)]) == BAD
    # the largest sizes that pass, and empty capacities
    assert stub.afsk_live_segments_layout((1 << 16) - 1, 1 << 15, 2 ** 31 - 1, 2 ** 31 - 1, *refs) == 0
    assert stub.afsk_live_segments_layout(1, 1, 0, 0, *refs) == 0
    assert [o.value for o in out] == [32, 32, 48]


def test_pack_argument_checks(stub):
    b = TapPush(stub)
    before = last_kernel(stub)[0]
    for change in (dict(n_channels=0), dict(n_channels=-3), dict(slots=0), dict(slots=-1),
                   dict(n_channels=1 << 16, slots=1 << 15), dict(max_segments=-1), dict(max_bytes=-1),
                   dict(max_bytes=2 ** 31), dict(tap_cap=0), dict(tap_cap=-4), dict(segments=b.sg_ptr + 4),
                   dict(segments=b.sg_ptr + 8)):
        assert stub.afsk_live_pack_tap(*b.seg_args(**change)) == BAD, change
    for ptr in ("n_closed", "burst_start", "burst_len", "flags", "nbytes", "tap_bytes", "tap_n", "tap_len",
                "open_start", "open_nbytes", "segments"):
        assert stub.afsk_live_pack_tap(*b.seg_args(**{ptr: None})) == BAD, ptr
    assert last_kernel(stub)[0] == before                                  # nothing was launched
    # empty capacities are fine
    assert stub.afsk_live_pack_tap(*b.seg_args()) == 0
    assert stub.afsk_live_pack_tap(*b.seg_args(max_segments=0, max_bytes=0)) == 0
    n, name, grid = last_kernel(stub)
    assert n == before + 6 and name == PACK_KERNELS[2] and grid == (N + 255) // 256


def test_a_pack_launches_its_three_kernels_in_order_and_nothing_else(logged):
    b = TapPush(logged)
    launches(logged)
    assert logged.afsk_live_pack_tap(*b.seg_args()) == 0
    assert launches(logged) == PACK_KERNELS
    one = TapPush(logged, n=1, slots=3, cap=1, max_segments=0, max_bytes=0)
    assert logged.afsk_live_pack_tap(*one.seg_args()) == 0
    assert launches(logged) == PACK_KERNELS
    # the two packers share the scan kernel and nothing else: neither launches the other's total or write kernel
    assert PACK_KERNELS[1] == EVENT_KERNELS[1]
    assert PACK_KERNELS[0] != EVENT_KERNELS[0] and PACK_KERNELS[2] != EVENT_KERNELS[2]
    assert ["LiveSegmentsArgs" in k for k in PACK_KERNELS] == [True, False, True]
    assert not any("LiveEventsArgs" in k for k in PACK_KERNELS)


@pytest.mark.parametrize("ragged", [False, True])
def test_the_tapped_push_then_the_pack_launch_the_pushs_kernels_then_the_packs(logged, ragged):
    """At the C level, the calls ``LiveReceiver.push(segments=)`` makes in its order -- with ``events=`` too: the event
    pack in between -- and the one call a push without either makes (the stub library cannot hold torch tensors: the
    Python glue itself runs in the GPU tests)."""
    n = 6
    bf = np.ascontiguousarray([40, 160] * (n // 2), np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    thr = lambda v: np.full(n, v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    h = C.c_void_p()
    assert logged.afsk_live_create_stream_tap(n, bf, thr(18000), thr(14000), STRIDE, T, C.byref(h)) == 0
    b = TapPush(logged, n=n)
    lens = np.full(n, T // 2, np.int32)

    def push():
        if ragged:
            a = b.tapped_push_args(h)
            assert logged.afsk_live_push_ragged(*a[:4], lens.ctypes.data, a[4], None, *a[5:]) == 0
        else:
            assert logged.afsk_live_push_tap(*b.tapped_push_args(h)) == 0

    launches(logged)
    push()
    alone = launches(logged)
    assert len(alone) == 1 and push_cell(alone[0]) == ("tap", False, ragged)
    push()
    assert logged.afsk_live_pack_tap(*b.seg_args()) == 0
    assert launches(logged) == alone + PACK_KERNELS
    push()
    assert logged.afsk_live_pack(*b.pack_args()) == 0
    assert logged.afsk_live_pack_tap(*b.seg_args()) == 0
    assert launches(logged) == alone + EVENT_KERNELS + PACK_KERNELS
    # and a push alone still launches what it launched
    push()
    assert launches(logged) == alone
    assert logged.afsk_live_destroy(h) == 0
