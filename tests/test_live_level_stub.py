"""The level tracker's C entries through the stub HIP runtime (no GPU): the host code of afsk_gate.hip built against
tests/helpers (build_stub_live_lib.sh, loaded through tests/stub_lib.py: a launch records the kernel's name and, when
asked, a copy of its first argument instead of running).  The return codes of afsk_live_create_stream_leveled,
afsk_live_level and afsk_live_level_reset, one live_level_kernel launch per call with a wave per channel, no launch
without samples, the parameters passed BY VALUE, a leveled receiver's pushes in the PER_CHANNEL cells although all pairs
agree, and the receivers of the existing create entries still launching the cells they did."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native
from afskmodem_amd.live import LevelSpec
from tests import stub_lib
from tests.live_push_cells import push_cell
from tests.stub_lib import i32, last_error, last_kernel

N, T, SLOTS, TAP_CAP = 6, 6144, 2, 800
GRID = (N + 3) // 4
_AUTO = re.compile(r"_ZN4afsk16live_push_kernelINS_13LiveAutoSinkTILb([01])EEELb([01])ELb([01])EEEv")
_MUTE = re.compile(r"_ZN4afsk21live_push_mute_kernelINS_15LiveStreamSinkTILb([01])EEELb([01])EEEv")
DEFAULT = LevelSpec().native()


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_level",
                         [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                          _native.LIVE_TAP_SIGNATURES, _native.LIVE_AUTO_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES,
                          _native.LIVE_CSMA_SIGNATURES, _native.LIVE_LEVEL_SIGNATURES])


def Buffers():
    return stub_lib.Buffers(N, T, SLOTS, TAP_CAP)


def create_leveled(lib, auto=False, tap=0, rates=None):
    (_, bf), (_, cand) = i32(rates or [40] * N), i32([40, 160, 8])
    (_, s), (_, e) = i32([18000] * N), i32([14000] * N)
    h = C.c_void_p()
    assert lib.afsk_live_create_stream_leveled(N, None if auto else bf, cand if auto else None, 3 if auto else 0, -1,
                                               s, e, 64, T, tap, C.byref(h)) == 0, last_error(lib)
    assert h
    return h


def create_others(lib):
    """A stored receiver, and the streaming / tapped / auto receivers of the existing entries, all with equal pairs."""
    (_, bf), (_, s), (_, e), (_, cand) = i32([40] * N), i32([18000] * N), i32([14000] * N), i32([40, 160])
    out = []
    for create, args in ((lib.afsk_live_create_thresholds, (N, bf, s, e, 48000, T)),
                         (lib.afsk_live_create_stream_thresholds, (N, bf, s, e, 64, T)),
                         (lib.afsk_live_create_stream_tap, (N, bf, s, e, 64, T)),
                         (lib.afsk_live_create_stream_auto, (N, cand, 2, -1, s, e, 64, T, 0))):
        h = C.c_void_p()
        assert create(*args, C.byref(h)) == 0
        out.append(h)
    return out


def level_args(h, state, chunk, params=DEFAULT, chunk_len=T, stride=T, lens=None, mute=None):
    return [h, None if state is None else state.ctypes.data, params, None if chunk is None else chunk.ctypes.data,
            stride, chunk_len, None if lens is None else lens.ctypes.data, None if mute is None else mute.ctypes.data,
            None]


def test_create_return_codes(stub):
    (_, bf), (_, cand), (_, s), (_, e) = i32([40] * N), i32([40, 160]), i32([18000] * N), i32([14000] * N)
    h = C.c_void_p(1234)
    bad, baud = _native.E_INVALID_ARG, _native.E_INVALID_BAUD
    for args in ((0, bf, None, 0, -1, s, e, 64, T, 0), (N, None, None, 0, -1, s, e, 64, T, 0),
                 (N, bf, None, 2, -1, s, e, 64, T, 0), (N, bf, cand, -1, -1, s, e, 64, T, 0),
                 (N, bf, cand, 37, -1, s, e, 64, T, 0), (N, bf, None, 0, -1, None, e, 64, T, 0),
                 (N, bf, None, 0, -1, s, None, 64, T, 0), (N, bf, None, 0, -1, s, e, -1, T, 0),
                 (N, bf, None, 0, -1, s, e, 65537, T, 1), (N, bf, None, 0, -1, s, e, 64, 0, 0),
                 (N, bf, None, 0, -1, s, e, 64, T, 2)):
        assert stub.afsk_live_create_stream_leveled(*args, C.byref(h)) == bad, args
        assert not h
    assert stub.afsk_live_create_stream_leveled(N, bf, None, 0, -1, s, e, 64, T, 0, None) == bad
    _, odd = i32([40, 42] * (N // 2))
    assert stub.afsk_live_create_stream_leveled(N, odd, None, 0, -1, s, e, 64, T, 0, C.byref(h)) == baud
    assert stub.afsk_live_create_stream_leveled(N, None, odd, 2, -1, s, e, 64, T, 0, C.byref(h)) == baud
    # the state is the per-channel streaming layout: two more int32 arrays than the one-pair receiver's
    lv, plain = create_leveled(stub), create_others(stub)[1]
    a, b = C.c_int64(), C.c_int64()
    assert stub.afsk_live_info(lv, None, None, C.byref(a)) == 0 and stub.afsk_live_info(plain, None, None, C.byref(b)) == 0
    assert a.value >= b.value
    for x in (lv, plain):
        assert stub.afsk_live_destroy(x) == 0


def test_level_and_reset_return_codes(stub):
    state, chunk = np.zeros((N, 4), np.int32), np.zeros((N, T), np.int16)
    lv = create_leveled(stub)
    others = create_others(stub)
    before = last_kernel(stub)[0]
    bad = _native.E_INVALID_ARG
    for h in others:                                        # a stored receiver, receivers of the other create entries
        assert stub.afsk_live_level(*level_args(h, state, chunk)) == bad
        assert stub.afsk_live_level_reset(h, state.ctypes.data, None, 18000, 14000, None) == bad
    assert "stored" in last_error(stub) or "afsk_live_create_stream_leveled" in last_error(stub)
    assert stub.afsk_live_level(*level_args(others[0], state, chunk)) == bad and "stored" in last_error(stub)
    assert stub.afsk_live_level(*level_args(others[1], state, chunk)) == bad
    assert "afsk_live_create_stream_leveled" in last_error(stub)
    assert stub.afsk_live_level(*level_args(None, state, chunk)) == bad
    assert stub.afsk_live_level(*level_args(lv, None, chunk)) == bad
    assert stub.afsk_live_level(*level_args(lv, state, None)) == bad
    assert stub.afsk_live_level(*level_args(lv, state, chunk, chunk_len=-1)) == bad
    assert stub.afsk_live_level(*level_args(lv, state, chunk, chunk_len=T + 1)) == bad
    assert stub.afsk_live_level(*level_args(lv, state, chunk, stride=-1)) == bad
    for kw in (dict(end_q15=18001), dict(start_q15=65536), dict(floor_end_q8=-1), dict(min_end=1025),
               dict(decay_shift=16), dict(rise_shift=-1)):
        params = _native.LiveLevelParams(*(dict(zip(LevelSpec.FIELDS, (getattr(DEFAULT, f) for f in LevelSpec.FIELDS)),
                                                **kw)[f] for f in LevelSpec.FIELDS))
        assert stub.afsk_live_level(*level_args(lv, state, chunk, params=params)) == bad, kw
        assert stub.afsk_live_level_check(params) == bad
    assert stub.afsk_live_level_check(DEFAULT) == 0
    assert stub.afsk_live_level_reset(None, state.ctypes.data, None, 18000, 14000, None) == bad
    assert stub.afsk_live_level_reset(lv, None, None, 18000, 14000, None) == bad
    assert last_kernel(stub)[0] == before                               # nothing was launched
    for h in [lv] + others:
        assert stub.afsk_live_destroy(h) == 0


def test_one_launch_per_call_a_wave_per_channel_and_none_without_samples(stub):
    state, chunk = np.zeros((N, 4), np.int32), np.zeros((N, T), np.int16)
    lens, mute = np.full(N, 100, np.int32), np.zeros((N, 2), np.int32)
    for auto, tap in ((False, 0), (False, 1), (True, 0), (True, 1)):
        lv = create_leveled(stub, auto=auto, tap=tap)
        for kw in (dict(), dict(lens=lens), dict(mute=mute), dict(lens=lens, mute=mute), dict(chunk_len=1),
                   dict(stride=0)):
            before = last_kernel(stub)[0]
            assert stub.afsk_live_level(*level_args(lv, state, chunk, **kw)) == 0, kw
            n, name, grid = last_kernel(stub)
            assert n == before + 1 and grid == GRID and "live_level_kernel" in name, (name, kw)
        before = last_kernel(stub)[0]
        assert stub.afsk_live_level(*level_args(lv, state, chunk, chunk_len=0)) == 0
        assert stub.afsk_live_level(*level_args(lv, state, None, chunk_len=0)) == 0     # no chunk needed
        assert last_kernel(stub)[0] == before
        mask = np.ones(N, np.uint8)
        for m in (None, mask.ctypes.data):
            assert stub.afsk_live_level_reset(lv, state.ctypes.data, m, 18000, 14000, None) == 0
            n, name, grid = last_kernel(stub)
            assert n == before + 1 and grid == 1 and "live_level_reset_kernel" in name
            before = n
        assert stub.afsk_live_reset(lv, None, None) == 0 and "live_stream_reset_kernel" in last_kernel(stub)[1]
        assert stub.afsk_live_destroy(lv) == 0


def test_the_parameters_travel_by_value(stub):
    lv = create_leveled(stub)
    state, chunk = np.zeros((N, 4), np.int32), np.zeros((N, T), np.int16)
    params = _native.LiveLevelParams(17001, 13001, 601, 401, 1101, 801, 3, 5)
    size = 9 * 8 + 2 * 4 + 8 * 4
    stub.afsk_stub_capture_arg0(size)
    try:
        assert stub.afsk_live_level(*level_args(lv, state, chunk, params=params, chunk_len=T - 2, stride=T)) == 0
        buf = C.create_string_buffer(size)
        assert stub.afsk_stub_last_arg0(buf, size) == size
    finally:
        stub.afsk_stub_capture_arg0(0)
    raw = buf.raw
    tail = np.asarray([T - 2, N, 17001, 13001, 601, 401, 1101, 801, 3, 5], np.int32).tobytes()
    assert raw.endswith(tail)
    words = np.frombuffer(raw[: 9 * 8], np.uint64).tolist()
    assert chunk.ctypes.data in words and state.ctypes.data in words and T in words
    assert stub.afsk_live_destroy(lv) == 0


def test_a_leveled_receiver_pushes_through_the_per_channel_cells(stub):
    b = Buffers()
    mute = np.zeros((N, 2), np.int32)
    lv = create_leveled(stub)
    assert stub.afsk_live_push(*b.plain(lv)) == 0
    assert push_cell(last_kernel(stub)[1]) == ("stream", True, False)
    assert stub.afsk_live_push_ragged(*b.ragged(lv, lens=True)) == 0
    assert push_cell(last_kernel(stub)[1]) == ("stream", True, True)
    args = b.ragged(lv, lens=True)
    assert stub.afsk_live_push_muted(*args[:7], mute.ctypes.data, *args[7:]) == 0
    assert _MUTE.match(last_kernel(stub)[1]).groups() == ("0", "1")
    assert stub.afsk_live_destroy(lv) == 0
    tapped = create_leveled(stub, tap=1, rates=[40, 160] * (N // 2))
    assert stub.afsk_live_push_tap(*b.tapped(tapped)) == 0
    assert push_cell(last_kernel(stub)[1]) == ("tap", True, False)
    assert stub.afsk_live_destroy(tapped) == 0
    for tap in (0, 1):
        auto = create_leveled(stub, auto=True, tap=tap)
        assert stub.afsk_live_push_auto(*b.auto(auto, taps=bool(tap))) == 0
        assert _AUTO.match(last_kernel(stub)[1]).groups() == (str(tap), "1", "0")
        assert stub.afsk_live_push(*b.plain(auto)) == _native.E_INVALID_ARG    # an auto receiver keeps its push entry
        assert stub.afsk_live_destroy(auto) == 0


def test_receivers_of_the_existing_entries_launch_what_they_did(stub):
    b = Buffers()
    stored, stream, tapped, auto = create_others(stub)
    stub_lib.launches(stub)
    assert stub.afsk_live_push(*b.plain(stored)) == 0
    log = stub_lib.launches(stub)
    # (the gate, the clear of out_corrected, the demodulator over the slots)
    assert push_cell(log[0]) == ("stored", False, False) and log[-1] == "demod" and len(log) == 3
    assert "clear_i32_kernel" in log[1]
    assert stub.afsk_live_push(*b.plain(stream)) == 0
    assert stub.afsk_live_push_ragged(*b.ragged(stream, lens=True)) == 0
    assert stub.afsk_live_push_tap(*b.tapped(tapped)) == 0
    assert [push_cell(x) for x in stub_lib.launches(stub)] == [("stream", False, False), ("stream", False, True),
                                                               ("tap", False, False)]
    assert stub.afsk_live_push_auto(*b.auto(auto)) == 0
    log = stub_lib.launches(stub)
    assert len(log) == 1 and _AUTO.match(log[0]).groups() == ("0", "0", "0")
    for h in (stored, stream, tapped, auto):
        assert stub.afsk_live_destroy(h) == 0
