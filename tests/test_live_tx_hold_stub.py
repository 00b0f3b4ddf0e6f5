"""Carrier sense through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's name instead of
running): a hold pull is two launches and they are the hold forms, for a uniform, a mixed and a rated transmitter;
their plain and ragged pulls still launch what they launched; afsk_live_busy is one launch for every receiver kind;
and every refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import i32, last_error, last_kernel, launches_decoded

N, T, DEPTH, MAXP = 6, 6144, 4, 64


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_tx_hold",
                         [_native.LIVE_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_THRESHOLD_SIGNATURES,
                          _native.LIVE_TAP_SIGNATURES, _native.LIVE_AUTO_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                          _native.LIVE_MIXED_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES,
                          _native.LIVE_TX_RATED_SIGNATURES, _native.LIVE_TX_HOLD_SIGNATURES])


# kind -> (bit_frames per channel or the rate table, plain tile kernel, ragged tile kernel, hold tile kernel)
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


class Args:
    """Host memory standing in for the device arrays of a pull."""

    def __init__(self):
        self.out = np.zeros((N, T), np.int16)
        self.pending = np.zeros(N, np.int32)
        self.deferred = np.zeros(N, np.int64)
        self.lens = np.full(N, T // 2, np.int32)
        self.hold = np.ones(N, np.int32)

    def hold_pull(self, h, lens=True, hold=True, holdoff=4800, deferred=True, T=T):
        return [h, self.out.ctypes.data if T else None, T, T, self.lens.ctypes.data if lens else None,
                self.hold.ctypes.data if hold else None, holdoff, self.pending.ctypes.data,
                self.deferred.ctypes.data if deferred else None, None]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_hold_pull_is_two_launches_of_the_hold_forms(stub, kind):
    _, tile, tile_ragged, tile_hold = KINDS[kind]
    h, a = create_tx(stub, kind), Args()
    o, pd, ln = a.out.ctypes.data, a.pending.ctypes.data, a.lens.ctypes.data
    launches_decoded(stub)
    for lens in (True, False):
        for hold in (True, False):                                      # a NULL hold: nobody held, the same kernels
            assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, lens, hold)) == 0
            assert launches_decoded(stub) == [tile_hold, "live_tx_commit_hold_kernel"]
            assert last_kernel(stub)[2] == 1                            # the commit: one block of 256 for 6 channels
    assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, holdoff=0)) == 0
    assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, holdoff=_native.MAX_STREAM_LEN)) == 0
    assert launches_decoded(stub) == [tile_hold, "live_tx_commit_hold_kernel"] * 2
    assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, T=0)) == 0       # nothing to render: the commit alone
    assert launches_decoded(stub) == ["live_tx_commit_hold_kernel"]
    # the plain and the ragged pull launch what they launched
    assert stub.afsk_live_tx_pull(h, o, T, T, pd, None) == 0
    assert launches_decoded(stub) == [tile, "live_tx_commit_kernel"]
    for d_lens in (ln, None):
        assert stub.afsk_live_tx_pull_ragged(h, o, T, T, d_lens, pd, None) == 0
        assert launches_decoded(stub) == [tile_ragged, "live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_reset(h, None, pd, None) == 0
    assert launches_decoded(stub) == ["live_tx_reset_kernel"]
    assert stub.afsk_live_tx_destroy(h) == 0


def test_refusals_launch_nothing(stub):
    h, a = create_tx(stub, "uniform_1200"), Args()
    bad = _native.E_INVALID_ARG
    launches_decoded(stub)
    assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, deferred=False)) == bad
    assert "out_deferred" in last_error(stub)
    for holdoff in (-1, _native.MAX_STREAM_LEN + 1, -2 ** 31, 2 ** 31 - 1):
        assert stub.afsk_live_tx_pull_hold(*a.hold_pull(h, holdoff=holdoff)) == bad, holdoff
        assert "holdoff" in last_error(stub)
    assert stub.afsk_live_tx_pull_hold(*a.hold_pull(None)) == bad
    assert "null live transmitter" in last_error(stub)
    # the argument checks of afsk_live_tx_pull
    args = a.hold_pull(h)
    args[3] = -1
    assert stub.afsk_live_tx_pull_hold(*args) == bad
    args = a.hold_pull(h)
    args[2] = T - 1                                                     # rows would overlap
    assert stub.afsk_live_tx_pull_hold(*args) == bad
    args = a.hold_pull(h)
    args[1] = None
    assert stub.afsk_live_tx_pull_hold(*args) == bad
    args = a.hold_pull(h)
    args[7] = None                                                      # no out_pending
    assert stub.afsk_live_tx_pull_hold(*args) == bad
    args = a.hold_pull(h)
    args[3] = _native.MAX_STREAM_LEN + 1
    assert stub.afsk_live_tx_pull_hold(*args) == bad
    assert launches_decoded(stub) == []
    assert not a.out.any() and not a.pending.any() and not a.deferred.any()
    assert stub.afsk_live_tx_destroy(h) == 0


def create_rx(lib, kind):
    uniform, mixed = [40] * N, [40, 160] * (N // 2)
    two = [14000, 9000] * (N // 2)
    s = i32([18000] * N)[1]
    h = C.c_void_p()
    if kind == "stored":
        rc = lib.afsk_live_create(N, 40, 18000, 14000, 48000, T, C.byref(h))
    elif kind == "stored_thr":
        rc = lib.afsk_live_create_thresholds(N, i32(uniform)[1], s, i32(two)[1], 48000, T, C.byref(h))
    elif kind == "stored_mixed":
        rc = lib.afsk_live_create_mixed(N, i32(mixed)[1], 18000, 14000, 48000, T, C.byref(h))
    elif kind == "stream":
        rc = lib.afsk_live_create_stream(N, i32(mixed)[1], 18000, 14000, 64, T, C.byref(h))
    elif kind == "stream_thr":
        rc = lib.afsk_live_create_stream_thresholds(N, i32(mixed)[1], s, i32(two)[1], 64, T, C.byref(h))
    else:
        assert kind == "tap"
        rc = lib.afsk_live_create_stream_tap(N, i32(mixed)[1], s, i32(two)[1], 0, T, C.byref(h))
    assert rc == 0 and h
    return h


@pytest.mark.parametrize("kind", ["stored", "stored_thr", "stored_mixed", "stream", "stream_thr", "tap"])
def test_busy_is_one_launch_for_every_receiver_kind(stub, kind):
    h = create_rx(stub, kind)
    busy = np.full(N, 7, np.int32)
    launches_decoded(stub)
    assert stub.afsk_live_busy(h, busy.ctypes.data, None) == 0
    assert launches_decoded(stub) == ["live_busy_kernel"]
    assert last_kernel(stub)[2] == 1
    assert stub.afsk_live_busy(h, None, None) == _native.E_INVALID_ARG
    assert stub.afsk_live_busy(None, busy.ctypes.data, None) == _native.E_INVALID_ARG
    assert "null live receiver" in last_error(stub)
    assert launches_decoded(stub) == []
    assert (busy == 7).all()                                            # (a stub launch runs nothing)
    assert stub.afsk_live_destroy(h) == 0
