"""The half-duplex entries through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's name
instead of running): a csma pull is two launches -- the hold pull's tile kernel and live_tx_commit_csma_kernel -- for a
uniform, a mixed and a rated transmitter; a muted push is one launch of live_push_mute_kernel<Sink, PER_CHANNEL> of the
receiver's sink and threshold form, plus the stored receiver's demodulator; the plain, ragged and hold pulls and pushes
still launch what they launched; and every refusal launches nothing and names the entry."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import i32, last_error, last_kernel, launches, launches_decoded

N, T, DEPTH, MAXP = 6, 6144, 4, 64
SLOTS, TAP_CAP = 2, 800

_MUTE = re.compile(r"_ZN4afsk21live_push_mute_kernelINS_(13LiveStoreSink|15LiveStreamSinkTILb([01])EE|"
                   r"13LiveAutoSinkTILb([01])EE)ELb([01])EEEvNT_4ArgsENS_12LivePushPtrsEPKi$")
_AUTO = re.compile(r"_ZN4afsk16live_push_kernelINS_13LiveAutoSinkTILb([01])EEELb([01])ELb([01])EEEv")


def mute_cell(mangled):
    """(sink, per_channel) of a live_push_mute_kernel instantiation's mangled name, None for any other kernel."""
    m = _MUTE.match(mangled)
    if not m:
        assert "live_push_mute_kernel" not in mangled, mangled
        return None
    sink = "stored" if m.group(1) == "13LiveStoreSink" else \
        ("stream", "tap")[int(m.group(2))] if m.group(2) is not None else ("auto", "auto_tap")[int(m.group(3))]
    return sink, m.group(4) == "1"


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_csma",
                         [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                          _native.LIVE_TAP_SIGNATURES, _native.LIVE_AUTO_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                          _native.LIVE_MIXED_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES,
                          _native.LIVE_TX_RATED_SIGNATURES, _native.LIVE_TX_HOLD_SIGNATURES,
                          _native.LIVE_CSMA_SIGNATURES])


# ------------------------------------------------------------------------------------------------------ the pull

# kind -> (bit_frames per channel or the rate table, plain, ragged and hold tile kernel)
KINDS = {"uniform_1200": ([40] * N, "live_tx_tile_kernel<0>", "live_tx_tile_ragged_kernel<0>",
                          "live_tx_tile_hold_kernel<0>"),
         "uniform_6000": ([8] * N, "live_tx_tile_kernel<1>", "live_tx_tile_ragged_kernel<1>",
                          "live_tx_tile_hold_kernel<1>"),
         "mixed": ([160, 40, 8] * (N // 3), "live_tx_tile_kernel_mixed", "live_tx_tile_ragged_kernel_mixed",
                   "live_tx_tile_hold_kernel_mixed"),
         "rated": ([160, 40, 20], "live_tx_tile_kernel_rated", "live_tx_tile_ragged_kernel_rated",
                   "live_tx_tile_hold_kernel_rated")}


def create_tx(lib, kind):
    h = C.c_void_p()
    bfs = KINDS[kind][0]
    if kind == "rated":
        rc = lib.afsk_live_tx_create_rated(N, len(bfs), i32(bfs)[1], i32([10] * len(bfs))[1], DEPTH, MAXP, C.byref(h))
    else:
        rc = lib.afsk_live_tx_create_mixed(N, i32(bfs)[1], i32([10] * N)[1], DEPTH, MAXP, C.byref(h))
    assert rc == 0 and h
    return h


class PullArgs:
    """Host memory standing in for the device arrays of a pull."""

    def __init__(self):
        self.out = np.zeros((N, T), np.int16)
        self.pending = np.zeros(N, np.int32)
        self.deferred = np.zeros(N, np.int64)
        self.on_air = np.zeros((N, 2), np.int32)
        self.lens = np.full(N, T // 2, np.int32)
        self.hold = np.ones(N, np.int32)

    def csma(self, h, lens=True, hold=True, holdoff=4800, persist=63, slot=4800, seed=7, deferred=True, on_air=True,
             T=T):
        return [h, self.out.ctypes.data if T else None, T, T, self.lens.ctypes.data if lens else None,
                self.hold.ctypes.data if hold else None, holdoff, persist, slot, seed, self.pending.ctypes.data,
                self.deferred.ctypes.data if deferred else None, self.on_air.ctypes.data if on_air else None, None]

    def held(self, h):
        return [h, self.out.ctypes.data, T, T, self.lens.ctypes.data, self.hold.ctypes.data, 4800,
                self.pending.ctypes.data, self.deferred.ctypes.data, None]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_csma_pull_is_the_hold_tile_kernel_and_the_csma_commit(stub, kind):
    _, tile, tile_ragged, tile_hold = KINDS[kind]
    h, a = create_tx(stub, kind), PullArgs()
    o, pd, ln = a.out.ctypes.data, a.pending.ctypes.data, a.lens.ctypes.data
    launches_decoded(stub)
    for lens in (True, False):
        for hold in (True, False):                                      # a NULL hold: nobody held, the same kernels
            assert stub.afsk_live_tx_pull_csma(*a.csma(h, lens, hold)) == 0
            assert launches_decoded(stub) == [tile_hold, "live_tx_commit_csma_kernel"]
            assert last_kernel(stub)[2] == 1                            # the commit: one block of 256 for 6 channels
    for kw in (dict(persist=0, slot=0, seed=0), dict(persist=255, slot=2 ** 20, seed=2 ** 32 - 1),
               dict(holdoff=_native.MAX_STREAM_LEN)):
        assert stub.afsk_live_tx_pull_csma(*a.csma(h, **kw)) == 0, kw
        assert launches_decoded(stub) == [tile_hold, "live_tx_commit_csma_kernel"]
    assert stub.afsk_live_tx_pull_csma(*a.csma(h, T=0)) == 0            # nothing to render: the commit alone
    assert launches_decoded(stub) == ["live_tx_commit_csma_kernel"]
    # the plain, the ragged and the hold pull launch what they launched
    assert stub.afsk_live_tx_pull(h, o, T, T, pd, None) == 0
    assert launches_decoded(stub) == [tile, "live_tx_commit_kernel"]
    assert stub.afsk_live_tx_pull_ragged(h, o, T, T, ln, pd, None) == 0
    assert launches_decoded(stub) == [tile_ragged, "live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_pull_hold(*a.held(h)) == 0
    assert launches_decoded(stub) == [tile_hold, "live_tx_commit_hold_kernel"]
    assert stub.afsk_live_tx_destroy(h) == 0


def test_pull_refusals_launch_nothing_and_name_the_entry(stub):
    h, a = create_tx(stub, "uniform_1200"), PullArgs()
    bad = _native.E_INVALID_ARG
    launches_decoded(stub)
    for kw, word in ((dict(persist=256), "persist"), (dict(persist=-1), "persist"), (dict(slot=2 ** 20 + 1), "slot"),
                     (dict(slot=-1), "slot"), (dict(on_air=False), "out_on_air")):
        assert stub.afsk_live_tx_pull_csma(*a.csma(h, **kw)) == bad, kw
        assert "afsk_live_tx_pull_csma" in last_error(stub) and word in last_error(stub), kw
    # the hold pull's checks
    assert stub.afsk_live_tx_pull_csma(*a.csma(h, deferred=False)) == bad
    assert "out_deferred" in last_error(stub)
    for holdoff in (-1, _native.MAX_STREAM_LEN + 1):
        assert stub.afsk_live_tx_pull_csma(*a.csma(h, holdoff=holdoff)) == bad
        assert "holdoff" in last_error(stub)
    assert stub.afsk_live_tx_pull_csma(*a.csma(None)) == bad
    assert "null live transmitter" in last_error(stub)
    args = a.csma(h)
    args[2] = T - 1                                                     # rows would overlap
    assert stub.afsk_live_tx_pull_csma(*args) == bad
    args = a.csma(h)
    args[10] = None                                                     # no out_pending
    assert stub.afsk_live_tx_pull_csma(*args) == bad
    assert launches_decoded(stub) == []
    assert not a.out.any() and not a.pending.any() and not a.deferred.any() and not a.on_air.any()
    assert stub.afsk_live_tx_destroy(h) == 0


# ------------------------------------------------------------------------------------------------------ the push

def create_rx(lib, kind, per_channel):
    bfs = i32([40, 160] * (N // 2))[1]
    s = i32([18000] * N)[1]
    e = i32([14000 - (c % 3 if per_channel else 0) for c in range(N)])[1]
    h = C.c_void_p()
    if kind == "stored":
        rc = lib.afsk_live_create_thresholds(N, bfs, s, e, 3 * 2048, T, C.byref(h))
    elif kind == "stream":
        rc = lib.afsk_live_create_stream_thresholds(N, bfs, s, e, 64, T, C.byref(h))
    elif kind == "tap":
        rc = lib.afsk_live_create_stream_tap(N, bfs, s, e, 64, T, C.byref(h))
    else:
        rc = lib.afsk_live_create_stream_auto(N, i32([40, 160, 8])[1], 3, -1, s, e, 64, T, int(kind == "auto_tap"),
                                              C.byref(h))
    assert rc == 0 and h
    return h


class PushArgs(stub_lib.Buffers):
    def __init__(self, slots):
        super().__init__(N, T, slots, TAP_CAP)
        self.mute = np.zeros((N, 2), np.int32)

    def muted(self, h, auto=False, mute=True, **kw):
        args = self.auto(h, **kw) if auto else self.ragged(h, **kw)
        return args[:7] + [self.mute.ctypes.data if mute else None] + args[7:]


def slots_of(lib, h):
    slots = C.c_int32()
    assert lib.afsk_live_info(h, None, C.byref(slots), None) == 0
    return slots.value


@pytest.mark.parametrize("per_channel", [False, True], ids=["one_pair", "pairs"])
@pytest.mark.parametrize("kind", ["stored", "stream", "tap", "auto", "auto_tap"])
def test_a_muted_push_is_one_launch_of_the_mute_kernel_of_its_sink(stub, kind, per_channel):
    h = create_rx(stub, kind, per_channel)
    b = PushArgs(slots_of(stub, h))
    auto, taps = kind.startswith("auto"), kind in ("tap", "auto_tap")
    entry = stub.afsk_live_push_auto_muted if auto else stub.afsk_live_push_muted
    launches(stub)
    for kw in (dict(), dict(lens=True), dict(mask=True), dict(lens=True, mask=True, flush=1), dict(chunk_len=0),
               dict(flush=1)):
        base = stub.afsk_live_push_auto if auto else stub.afsk_live_push_ragged
        assert base(*(b.auto if auto else b.ragged)(h, taps=taps, **kw)) == 0, kw
        behind = launches(stub)[1:]                                     # the stored receiver's demodulator launches
        assert bool(behind) == (kind == "stored") and (not behind or behind[-1] == "demod")
        assert entry(*b.muted(h, auto, taps=taps, **kw)) == 0, kw
        log = launches(stub)
        assert mute_cell(log[0]) == (kind, per_channel), (log, kw)
        assert log[1:] == behind, (log, kw)
    if taps:                                                            # without the tap outputs: the untapped sink
        assert entry(*b.muted(h, auto)) == 0
        assert mute_cell(launches(stub)[0]) == ({"tap": "stream", "auto_tap": "auto"}[kind], per_channel)
    # the entries without a mute launch what they launched
    if auto:
        for kw, ragged in ((dict(), False), (dict(lens=True), True)):
            assert stub.afsk_live_push_auto(*b.auto(h, taps=taps, **kw)) == 0
            (name,) = launches(stub)
            assert _AUTO.match(name).groups() == (str(int(taps)), str(int(per_channel)), str(int(ragged)))
    else:
        assert stub.afsk_live_push_ragged(*b.ragged(h, lens=True, taps=taps)) == 0
        assert launches_decoded(stub)[0] == (kind, per_channel, True)
        plain = stub.afsk_live_push_tap(*b.tapped(h)) if taps else stub.afsk_live_push(*b.plain(h))
        assert plain == 0 and launches_decoded(stub)[0] == (kind, per_channel, False)
    assert stub.afsk_live_destroy(h) == 0


def test_push_refusals_launch_nothing_and_name_the_entry(stub):
    bad = _native.E_INVALID_ARG
    fixed, auto = create_rx(stub, "stream", False), create_rx(stub, "auto", False)
    b = PushArgs(slots_of(stub, fixed))
    assert slots_of(stub, auto) == slots_of(stub, fixed)
    launches(stub)
    assert stub.afsk_live_push_muted(*b.muted(fixed, mute=False)) == bad
    assert "afsk_live_push_muted" in last_error(stub) and "d_mute" in last_error(stub)
    assert stub.afsk_live_push_auto_muted(*b.muted(auto, True, mute=False)) == bad
    assert "afsk_live_push_auto_muted" in last_error(stub) and "d_mute" in last_error(stub)
    # the auto entry on a fixed-rate receiver, and the reverse
    assert stub.afsk_live_push_auto_muted(*b.muted(fixed, True)) == bad
    assert last_error(stub).startswith("afsk_live_push_auto_muted needs") and "afsk_live_push_muted" in last_error(stub)
    assert stub.afsk_live_push_muted(*b.muted(auto)) == bad
    assert last_error(stub).startswith("afsk_live_push_muted:") and "afsk_live_push_auto_muted" in last_error(stub)
    # the ragged push's checks
    assert stub.afsk_live_push_muted(*b.muted(None)) == bad
    assert "null live receiver" in last_error(stub)
    assert stub.afsk_live_push_muted(*b.muted(fixed, chunk_len=T + 1)) == bad
    assert "max_chunk_len" in last_error(stub)
    assert stub.afsk_live_push_muted(*b.muted(fixed, chunk_len=-1)) == bad
    assert stub.afsk_live_push_muted(*b.muted(fixed, taps=True)) == bad            # tap outputs, no tapped receiver
    args = b.muted(fixed)
    args[8] = None                                                      # no out_n_closed
    assert stub.afsk_live_push_muted(*args) == bad
    args = b.muted(auto, True)
    args[-2] = None                                                     # no out_rate_score
    assert stub.afsk_live_push_auto_muted(*args) == bad
    assert launches(stub) == []
    assert stub.afsk_live_destroy(fixed) == 0 and stub.afsk_live_destroy(auto) == 0
