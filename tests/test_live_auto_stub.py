"""The auto-rate receiver's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built against
tests/helpers (build_stub_live_lib.sh, loaded through tests/stub_lib.py: a launch records the kernel's name and, when
asked, a copy of its first argument instead of running).  The return codes of afsk_live_create_stream_auto and
afsk_live_push_auto, which push entry serves which receiver, one launch per push and which cell of the push table it
is, the candidate list passed BY VALUE, and the fixed-rate receivers still launching the cells they did."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, batch
from tests import stub_lib
from tests.live_push_cells import push_cell
from tests.stub_lib import i32, last_error, last_kernel

N, T, SLOTS, TAP_CAP = 6, 6144, 2, 800
# what an auto cell's argument holds at least: the streaming sink's argument (232 bytes; with the tap's 280), then two
# pointers, max_score, n_cand and 36 candidates
ARG_BYTES = {False: 232 + 16 + 8 + 144, True: 280 + 16 + 8 + 144}
_AUTO = re.compile(r"_ZN4afsk16live_push_kernelINS_13LiveAutoSinkTILb([01])EEELb([01])ELb([01])EEEv")


def auto_cell(mangled):
    """(tapped, per_channel, ragged) of an auto instantiation of live_push_kernel, None for any other kernel."""
    m = _AUTO.match(mangled)
    return tuple(g == "1" for g in m.groups()) if m else None


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_auto",
                         [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                          _native.LIVE_TAP_SIGNATURES, _native.LIVE_AUTO_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES])


def Buffers():
    """This module's sizes; a ragged or auto argument list passes neither lens nor mask unless told to."""
    return stub_lib.Buffers(N, T, SLOTS, TAP_CAP)


def create_auto(lib, cands=(40, 160, 8), max_score=-1, per_channel=False, tap=0, maxp=64):
    (keep, c), (_, s) = i32(cands), i32([18000] * N)
    _, e = i32([14000 - (c % 3 if per_channel else 0) for c in range(N)])
    h = C.c_void_p()
    assert lib.afsk_live_create_stream_auto(N, c, len(cands), max_score, s, e, maxp, T, tap, C.byref(h)) == 0
    assert h
    return h, keep


def test_create_return_codes(stub):
    (_, c), (_, s), (_, e) = i32([40, 160]), i32([18000] * N), i32([14000] * N)
    h = C.c_void_p(1234)
    bad, baud = _native.E_INVALID_ARG, _native.E_INVALID_BAUD
    for args in ((0, c, 2, -1, s, e, 64, T, 0), (N, None, 2, -1, s, e, 64, T, 0), (N, c, 0, -1, s, e, 64, T, 0),
                 (N, c, -1, -1, s, e, 64, T, 0), (N, c, 2, -1, None, e, 64, T, 0), (N, c, 2, -1, s, None, 64, T, 0),
                 (N, c, 2, -1, s, e, -1, T, 0), (N, c, 2, -1, s, e, 65537, T, 0), (N, c, 2, -1, s, e, 64, 0, 0),
                 (N, c, 2, -1, s, e, 64, _native.MAX_STREAM_LEN + 1, 1), (N, c, 2, -1, s, e, 64, T, 2),
                 (N, c, 2, -1, s, e, 64, T, -1)):
        assert stub.afsk_live_create_stream_auto(*args, C.byref(h)) == bad, args
        assert not h
    _, many = i32(list(batch.VALID_BIT_FRAMES) + [40])
    assert stub.afsk_live_create_stream_auto(N, many, 37, -1, s, e, 64, T, 0, C.byref(h)) == bad
    assert stub.afsk_live_create_stream_auto(N, c, 2, -1, s, e, 64, T, 0, None) == bad
    for value in (0, 2, 6, 41, 2048, 4000, -40):
        _, one = i32([40, value, 80])
        assert stub.afsk_live_create_stream_auto(N, one, 3, -1, s, e, 64, T, 0, C.byref(h)) == baud, value
    # all 36 candidates, duplicates, a score limit, the largest capacities
    _, every = i32(batch.VALID_BIT_FRAMES)
    for cand, k, limit, tap in ((every, 36, -1, 0), (every, 36, 0, 1), (i32([40, 40, 160])[1], 3, 2 ** 31 - 1, 1)):
        assert stub.afsk_live_create_stream_auto(N, cand, k, limit, s, e, 65536, _native.MAX_STREAM_LEN, tap,
                                                 C.byref(h)) == 0
        assert stub.afsk_live_destroy(h) == 0


def test_the_state_is_the_streaming_layout_and_info_reset_destroy_serve_it(stub):
    for per_channel in (False, True):
        h, _ = create_auto(stub, per_channel=per_channel, tap=1, maxp=0)
        n, slots, nbytes = C.c_int32(), C.c_int32(), C.c_int64()
        assert stub.afsk_live_info(h, C.byref(n), C.byref(slots), C.byref(nbytes)) == 0
        want_slots, want_bytes = C.c_int32(), C.c_int64()
        assert stub.afsk_live_stream_layout(N, 0, T, C.byref(want_slots), C.byref(want_bytes)) == 0
        assert (n.value, slots.value) == (N, want_slots.value) and slots.value == SLOTS
        if not per_channel:
            assert nbytes.value == want_bytes.value
        assert stub.afsk_live_reset(h, None, None) == 0
        assert "live_stream_reset_kernel" in last_kernel(stub)[1]
        mask = np.ones(N, np.uint8)
        assert stub.afsk_live_reset(h, mask.ctypes.data, None) == 0
        assert stub.afsk_live_destroy(h) == 0


@pytest.mark.parametrize("tap", [0, 1], ids=["untapped", "tapped"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["one_pair", "pairs"])
def test_one_launch_per_push_and_the_cell_it_is(stub, per_channel, tap):
    h, _ = create_auto(stub, per_channel=per_channel, tap=tap)
    b = Buffers()
    names = set()
    for taps in ([False, True] if tap else [False]):
        for kw, ragged in ((dict(), False), (dict(lens=True), True), (dict(mask=True), True),
                           (dict(lens=True, mask=True, flush=1), True), (dict(chunk_len=0), False),
                           (dict(flush=1), False)):
            before = last_kernel(stub)[0]
            assert stub.afsk_live_push_auto(*b.auto(h, taps=taps, **kw)) == 0, kw
            n, name, grid = last_kernel(stub)
            assert n == before + 1 and grid == 2                       # ONE launch, a wave per channel
            assert auto_cell(name) == (taps, per_channel, ragged), (name, kw)
            assert "live_push_kernel" in name and "LiveAutoSinkT" in name
            names.add(name)
    assert len(names) == (4 if tap else 2)
    assert stub.afsk_live_destroy(h) == 0


def test_cross_use_is_refused_and_names_the_right_entry(stub):
    b = Buffers()
    h, _ = create_auto(stub, tap=1)
    before = last_kernel(stub)[0]
    bad = _native.E_INVALID_ARG
    assert stub.afsk_live_push(*b.plain(h)) == bad
    assert "afsk_live_push_auto" in last_error(stub)
    assert stub.afsk_live_push_tap(*b.plain(h)[:-1], *b.taps(), None) == bad
    assert "afsk_live_push_auto" in last_error(stub)
    assert stub.afsk_live_push_ragged(*b.ragged(h, lens=True)) == bad
    assert "afsk_live_push_auto" in last_error(stub)
    assert stub.afsk_live_destroy(h) == 0
    (_, bf), (_, s), (_, e) = i32([40, 160] * (N // 2)), i32([18000] * N), i32([14000] * N)
    others = []
    for create, cap in ((stub.afsk_live_create_stream_thresholds, 64), (stub.afsk_live_create_stream_tap, 64),
                        (stub.afsk_live_create_thresholds, 48000)):
        o = C.c_void_p()
        assert create(N, bf, s, e, cap, T, C.byref(o)) == 0
        others.append(o)
    for o in others:
        assert stub.afsk_live_push_auto(*b.auto(o)) == bad
        assert "afsk_live_create_stream_auto" in last_error(stub) and "afsk_live_push_ragged" in last_error(stub)
        assert stub.afsk_live_push_auto(*b.auto(o, taps=True, lens=True)) == bad
    assert last_kernel(stub)[0] == before                              # nothing was launched
    # a fixed-rate streaming receiver and a tapped one still launch the cells they did
    assert stub.afsk_live_push(*b.plain(others[0])) == 0
    assert push_cell(last_kernel(stub)[1]) == ("stream", False, False)
    assert stub.afsk_live_push_ragged(*b.ragged(others[0], lens=True)) == 0
    assert push_cell(last_kernel(stub)[1]) == ("stream", False, True)
    assert stub.afsk_live_push_tap(*b.plain(others[1])[:-1], *b.taps(), None) == 0
    assert push_cell(last_kernel(stub)[1]) == ("tap", False, False)
    assert stub.afsk_live_push(*b.plain(others[2])) == 0
    for o in others:
        assert stub.afsk_live_destroy(o) == 0


def test_push_auto_argument_checks(stub):
    h, _ = create_auto(stub, tap=1)
    untapped, _ = create_auto(stub, tap=0)
    b = Buffers()
    before = last_kernel(stub)[0]
    bad = _native.E_INVALID_ARG
    assert stub.afsk_live_push_auto(*b.auto(None)) == bad
    assert stub.afsk_live_push_auto(*b.auto(h, rates=(False, True))) == bad
    assert stub.afsk_live_push_auto(*b.auto(h, rates=(True, False))) == bad
    assert stub.afsk_live_push_auto(*b.auto(h, chunk_len=-1)) == bad
    assert stub.afsk_live_push_auto(*b.auto(h, chunk_len=T + 1)) == bad
    for missing in range(5):
        assert stub.afsk_live_push_auto(*b.auto(h, taps=True, missing=missing)) == bad, missing
    assert stub.afsk_live_push_auto(*b.auto(untapped, taps=True)) == bad   # tap outputs need tap = 1
    assert "tap = 1" in last_error(stub)
    margins = np.zeros(64, np.int32)
    assert stub.afsk_live_push_auto(*b.auto(h, margins=margins.ctypes.data)) == bad
    args = b.auto(h)
    args[7] = None                                                      # out_n_closed
    assert stub.afsk_live_push_auto(*args) == bad
    args = b.auto(h)
    args[1] = None                                                      # no chunk, chunk_len > 0
    assert stub.afsk_live_push_auto(*args) == bad
    assert last_kernel(stub)[0] == before
    args = b.auto(h, chunk_len=0)
    args[1] = None                                                      # chunk_len 0: no chunk needed
    assert stub.afsk_live_push_auto(*args) == 0
    assert last_kernel(stub)[0] == before + 1
    assert stub.afsk_live_destroy(h) == 0
    assert stub.afsk_live_destroy(untapped) == 0


@pytest.mark.parametrize("tap", [0, 1], ids=["untapped", "tapped"])
def test_the_candidate_list_travels_by_value_in_every_push(stub, tap):
    cands = [160, 8, 2000, 40, 40, 1920]
    h, keep = create_auto(stub, cands, max_score=1234, tap=tap)
    host_ptr = keep.ctypes.data
    keep[:] = -1                                        # the caller's array is its own again once create has returned
    b = Buffers()
    size = ARG_BYTES[bool(tap)]
    stub.afsk_stub_capture_arg0(size)
    try:
        assert stub.afsk_live_push_auto(*b.auto(h, taps=bool(tap))) == 0
        buf = C.create_string_buffer(size)
        assert stub.afsk_stub_last_arg0(buf, size) == size
    finally:
        stub.afsk_stub_capture_arg0(0)
    raw = buf.raw
    # max_score, n_cand and the list, back to back, behind the two output pointers
    tail = np.asarray([1234, len(cands)] + cands, np.int32).tobytes()
    at = raw.index(tail)
    assert at % 8 == 0 and at >= 16
    ptrs = np.frombuffer(raw[at - 16: at], np.uint64).tolist()
    assert ptrs == [b.rate[0].ctypes.data, b.rate[1].ctypes.data]
    words = np.frombuffer(raw[: at - at % 8], np.uint64).tolist()
    assert host_ptr not in words and b.chunk.ctypes.data in words
    if tap:
        assert b.tap[0].ctypes.data in words
    assert stub.afsk_live_destroy(h) == 0
