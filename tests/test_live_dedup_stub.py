"""The duplicate filter's C entries through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's
name instead of running): what every entry launches and in what order, the grids at the ``max_events`` / ``n_messages``
edges, that an empty call launches nothing, and every refusal -- which launches nothing and names its entry."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import i32, last_error, last_kernel, launches_decoded

BAD = _native.E_INVALID_ARG
ORDER, DEDUP, NOTE, RESET = "live_relay_order_kernel", "live_dedup_kernel", "live_dedup_note_kernel", \
    "live_dedup_reset_kernel"
TX_ORDER = "live_tx_order_kernel"
KEPT, KEPT_RATED = "live_relay_kept_kernel<0>", "live_relay_kept_kernel<1>"
N, DEPTH, ME, MB, STRIDE = 6, 8, 8, 64, 16


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_dedup",
                         [_native.LIVE_TX_SIGNATURES, _native.LIVE_MIXED_SIGNATURES, _native.LIVE_RELAY_SIGNATURES,
                          _native.LIVE_TX_RATED_SIGNATURES, _native.LIVE_DEDUP_SIGNATURES])


def create(lib, n=N, depth=DEPTH):
    h = C.c_void_p()
    assert lib.afsk_live_dedup_create(n, depth, C.byref(h)) == 0 and h, last_error(lib)
    return h


class Args:
    """Host memory standing in for the device arrays of a filter, a note and a kept relay."""

    def __init__(self):
        self.events = np.zeros(32 + 48 * ME + MB + 64, np.uint8)                 # (numpy data is 16-byte aligned)
        assert self.events.ctypes.data % 16 == 0
        self.verdict = np.full(ME, 9, np.int32)
        self.channels = np.arange(ME, dtype=np.int32) % N
        self.payload = np.zeros((ME, STRIDE), np.uint8)
        self.lens = np.full(ME, 3, np.int32)
        self.time = np.zeros(ME, np.int64)
        self.map = np.arange(N, dtype=np.int32)
        self.heard = np.zeros((N, 2), np.int32)
        self.keep = np.ones(ME, np.int32)
        self.out = (np.full(ME, 9, np.int32), np.full(ME, 9, np.int64), np.full(ME, 9, np.int32))

    def filter(self, h, **kw):
        a = dict(dd=h, events=self.events.ctypes.data, max_events=ME, max_bytes=MB, out_stride=STRIDE, skip=1, window=100,
                 verdict=self.verdict.ctypes.data, stream=None)
        a.update(kw)
        return list(a.values())

    def note(self, h, **kw):
        a = dict(dd=h, channels=self.channels.ctypes.data, payload=self.payload.ctypes.data, stride=STRIDE,
                 lens=self.lens.ctypes.data, time=self.time.ctypes.data, n=ME, window=100,
                 verdict=self.verdict.ctypes.data, stream=None)
        a.update(kw)
        return list(a.values())

    def kept(self, tx, heard=False, **kw):
        a = dict(tx=tx, events=self.events.ctypes.data, max_events=ME, max_bytes=MB, out_stride=STRIDE, n_rx=N,
                 map=None, skip=1, heard=self.heard.ctypes.data if heard else None, slots=2 if heard else 0,
                 keep=self.keep.ctypes.data, st=self.out[0].ctypes.data, start=self.out[1].ctypes.data,
                 ns=self.out[2].ctypes.data, stream=None)
        a.update(kw)
        return list(a.values())

    def untouched(self):
        return (self.verdict == 9).all() and all((o == 9).all() for o in self.out) and not self.events.any()


def transmitters(lib):
    """(kind, handle): a uniform, a mixed and a rated transmitter of N channels."""
    out = []
    for kind, bfs in (("uniform", [40] * N), ("mixed", [40, 8, 160, 40, 8, 160])):
        h = C.c_void_p()
        assert lib.afsk_live_tx_create_mixed(N, i32(bfs)[1], i32([10] * N)[1], 2, 32, C.byref(h)) == 0 and h
        out.append((kind, h))
    h = C.c_void_p()
    assert lib.afsk_live_tx_create_rated(N, 2, i32([40, 8])[1], i32([10, 0])[1], 2, 32, C.byref(h)) == 0 and h
    return out + [("rated", h)]


def test_create_empties_the_rings_with_one_launch_and_reports_its_layout(stub):
    launches_decoded(stub)
    h = create(stub)
    assert launches_decoded(stub) == [RESET]
    assert last_kernel(stub)[2] == 1                                            # 48 entries: one block of 256
    nbytes = C.c_int64()
    assert stub.afsk_live_dedup_layout(N, DEPTH, C.byref(nbytes)) == 0 and nbytes.value == 768 + 256 + 256
    # the state as create left it (the stub zeroes and runs no kernel): readable, writable, size-checked
    raw = np.full(nbytes.value - 256, 7, np.uint8)
    assert stub.afsk_live_dedup_get_state(h, raw.ctypes.data, raw.size) == 0 and not raw.any()
    raw[768: 768 + 4 * N].view(np.int32)[:] = DEPTH - 1
    assert stub.afsk_live_dedup_set_state(h, raw.ctypes.data, raw.size) == 0
    back = np.zeros_like(raw)
    assert stub.afsk_live_dedup_get_state(h, back.ctypes.data, back.size) == 0 and (back == raw).all()
    raw[768: 772].view(np.int32)[:] = DEPTH
    assert stub.afsk_live_dedup_set_state(h, raw.ctypes.data, raw.size) == BAD and "head" in last_error(stub)
    raw[768: 772].view(np.int32)[:] = -1
    assert stub.afsk_live_dedup_set_state(h, raw.ctypes.data, raw.size) == BAD
    for entry in (stub.afsk_live_dedup_get_state, stub.afsk_live_dedup_set_state):
        assert entry(h, raw.ctypes.data, raw.size - 1) == BAD and entry(h, raw.ctypes.data, nbytes.value) == BAD
        assert entry(h, None, raw.size) == BAD and entry(None, raw.ctypes.data, raw.size) == BAD
    assert launches_decoded(stub) == []
    assert stub.afsk_live_dedup_destroy(h) == 0 and stub.afsk_live_dedup_destroy(None) == 0


def test_create_and_layout_refusals(stub):
    launches_decoded(stub)
    for n, depth, word in ((0, 8, "n_channels"), (-3, 8, "n_channels"), (4, 0, "depth"), (4, 65, "depth"),
                           (4, -1, "depth")):
        h = C.c_void_p(77)
        assert stub.afsk_live_dedup_create(n, depth, C.byref(h)) == BAD and not h
        assert "afsk_live_dedup" in last_error(stub) and word in last_error(stub)
        assert stub.afsk_live_dedup_layout(n, depth, None) == BAD
    assert stub.afsk_live_dedup_create(4, 8, None) == BAD
    assert stub.afsk_live_dedup_layout(4, 64, None) == 0 and stub.afsk_live_dedup_layout(1, 1, None) == 0
    assert launches_decoded(stub) == []


def test_a_filter_is_the_order_kernel_and_the_dedup_kernel(stub):
    h, a = create(stub), Args()
    launches_decoded(stub)
    for kw in (dict(), dict(skip=0), dict(skip=3), dict(window=0), dict(window=2 ** 62), dict(out_stride=0),
               dict(max_bytes=0)):
        assert stub.afsk_live_dedup_filter(*a.filter(h, **kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == [ORDER, DEDUP], kw
    assert stub.afsk_live_dedup_filter(*a.filter(h, max_events=0)) == 0
    assert stub.afsk_live_dedup_filter(*a.filter(h, max_events=0, verdict=None, events=None)) == BAD       # checked first
    assert launches_decoded(stub) == []
    assert a.untouched()
    stub.afsk_live_dedup_destroy(h)


@pytest.mark.parametrize("count,grid", [(1, 1), (16, 1), (17, 2), (32, 2), (33, 3), (70000, 4375), (2 ** 31 - 1, 2 ** 27)])
def test_the_grids_are_one_wave_per_four_indices(stub, count, grid):
    h, a = create(stub), Args()
    launches_decoded(stub)
    assert stub.afsk_live_dedup_filter(*a.filter(h, max_events=count)) == 0        # (the stub touches no memory)
    n, name, got = last_kernel(stub)
    assert "live_dedup_kernel" in name and got == grid
    assert stub.afsk_live_dedup_note(*a.note(h, n=count)) == 0
    n, name, got = last_kernel(stub)
    assert "live_dedup_note_kernel" in name and got == grid
    for kind, tx in transmitters(stub)[::2]:
        assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, max_events=count)) == 0
        assert last_kernel(stub)[2] == grid, kind
        stub.afsk_live_tx_destroy(tx)
    assert launches_decoded(stub)[:4] == [ORDER, DEDUP, TX_ORDER, NOTE]
    stub.afsk_live_dedup_destroy(h)


def test_a_note_is_the_submit_order_kernel_and_the_note_kernel(stub):
    h, a = create(stub), Args()
    launches_decoded(stub)
    for kw in (dict(), dict(window=0), dict(stride=0), dict(n=1)):
        assert stub.afsk_live_dedup_note(*a.note(h, **kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == [TX_ORDER, NOTE], kw
    # nothing to note: no launch, and no pointer is looked at
    assert stub.afsk_live_dedup_note(*a.note(h, n=0)) == 0
    assert stub.afsk_live_dedup_note(*a.note(h, n=0, channels=None, payload=None, lens=None, time=None, verdict=None)) == 0
    assert launches_decoded(stub) == []
    for kw, word in ((dict(dd=None), "null"), (dict(channels=None), "null"), (dict(payload=None), "null"),
                     (dict(lens=None), "null"), (dict(time=None), "null"), (dict(verdict=None), "null"),
                     (dict(n=-1), "negative"), (dict(stride=-1), "negative"), (dict(window=-1), "window")):
        assert stub.afsk_live_dedup_note(*a.note(h, **kw)) == BAD, kw
        assert "afsk_live_dedup_note" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
    assert launches_decoded(stub) == [] and a.untouched()
    stub.afsk_live_dedup_destroy(h)


def test_filter_refusals_launch_nothing_and_name_the_entry(stub):
    h, a = create(stub), Args()
    launches_decoded(stub)
    p = a.events.ctypes.data
    for kw, word in ((dict(dd=None), "null"), (dict(events=None), "null"), (dict(verdict=None), "null"),
                     (dict(max_events=-1), "negative"), (dict(max_bytes=-1), "negative"), (dict(out_stride=-1), "negative"),
                     (dict(window=-1), "window"), (dict(window=-2 ** 63), "window"), (dict(skip=4), "skip_flags"),
                     (dict(skip=7), "skip_flags"), (dict(skip=-1), "skip_flags"), (dict(events=p + 8), "aligned"),
                     (dict(events=p + 4), "aligned"), (dict(events=p + 1), "aligned")):
        assert stub.afsk_live_dedup_filter(*a.filter(h, **kw)) == BAD, kw
        assert "afsk_live_dedup_filter" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
    assert launches_decoded(stub) == [] and a.untouched()
    stub.afsk_live_dedup_destroy(h)


def test_reset_is_one_launch_over_the_entries(stub):
    h = create(stub, n=70000, depth=3)
    mask = np.zeros(70000, np.uint8)
    launches_decoded(stub)
    for m in (None, mask.ctypes.data):
        assert stub.afsk_live_dedup_reset(h, m, None) == 0
        assert launches_decoded(stub) == [RESET]
        assert last_kernel(stub)[2] == (70000 * 3 + 255) // 256
    assert stub.afsk_live_dedup_reset(None, None, None) == BAD and "afsk_live_dedup_reset" in last_error(stub)
    assert launches_decoded(stub) == []
    stub.afsk_live_dedup_destroy(h)


def test_a_kept_submit_is_two_launches_on_every_kind_of_transmitter(stub):
    a = Args()
    for kind, tx in transmitters(stub):
        launches_decoded(stub)
        want = KEPT_RATED if kind == "rated" else KEPT
        assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx)) == 0, (kind, last_error(stub))
        assert launches_decoded(stub) == [ORDER, want], kind
        assert last_kernel(stub)[2] == 1
        assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, map=a.map.ctypes.data, skip=0)) == 0
        assert launches_decoded(stub) == [ORDER, want], kind
        if kind == "rated":
            assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, heard=True)) == 0
            assert launches_decoded(stub) == [ORDER, want]
            assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, heard=True, slots=0)) == BAD
            assert "rx_slots" in last_error(stub)
        else:                                                                   # the rated-only misuse
            assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, heard=True)) == BAD
            assert "afsk_live_tx_create_rated" in last_error(stub)
        # the plain entries still launch what they launched
        plain = a.kept(tx)
        del plain[8:11]
        assert stub.afsk_live_tx_submit_events(*plain) == 0
        assert launches_decoded(stub) == [ORDER, "live_relay_rated_kernel" if kind == "rated" else "live_relay_kernel"]
        assert stub.afsk_live_tx_submit_events_kept(*a.kept(tx, max_events=0)) == 0
        p = a.events.ctypes.data
        for kw, word in ((dict(tx=None), "null"), (dict(events=None), "null"), (dict(keep=None), "null"),
                         (dict(st=None), "null"), (dict(start=None), "null"), (dict(ns=None), "null"),
                         (dict(max_events=-1), "negative"), (dict(max_bytes=-1), "negative"),
                         (dict(out_stride=-1), "negative"), (dict(n_rx=0), "n_rx_channels"), (dict(skip=4), "skip_flags"),
                         (dict(events=p + 8), "aligned")):
            assert stub.afsk_live_tx_submit_events_kept(*a.kept(kw.pop("tx", tx), **kw)) == BAD, (kind, kw)
            assert "afsk_live_tx_submit_events_kept" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
        assert launches_decoded(stub) == [], kind
        assert stub.afsk_live_tx_destroy(tx) == 0
    assert a.untouched()
