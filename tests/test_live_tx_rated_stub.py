"""The rated live transmitter's C entries through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the
kernel's name instead of running): two launches per rated submit, relay and pull and the kernels they are, a uniform
and a mixed transmitter still launching what they launched, the _rated entries refused on a transmitter that is not
rated with nothing launched, info's state bytes -- and the ValueErrors of the Python layer that need no device."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import stub_lib
from tests.stub_lib import i32, last_error, last_kernel, launches_decoded

N, T, DEPTH, MAXP = 6, 6144, 4, 64


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_tx_rated",
                         [_native.LIVE_TX_SIGNATURES, _native.LIVE_MIXED_SIGNATURES, _native.LIVE_RAGGED_SIGNATURES,
                          _native.LIVE_RELAY_SIGNATURES, _native.LIVE_TX_RATED_SIGNATURES])


def create_rated(lib, bfs=(40, 8, 160), ts=(10, 0, 3)):
    h = C.c_void_p()
    assert lib.afsk_live_tx_create_rated(N, len(bfs), i32(bfs)[1], i32(ts)[1], DEPTH, MAXP, C.byref(h)) == 0 and h
    return h


def create_mixed(lib, bfs):
    h = C.c_void_p()
    assert lib.afsk_live_tx_create_mixed(N, i32(bfs)[1], i32([10] * N)[1], DEPTH, MAXP, C.byref(h)) == 0 and h
    return h


class Args:
    """Host memory standing in for the device arrays of a submit, a relay and a pull."""

    def __init__(self):
        self.mem = np.zeros(1 << 16, np.uint8)
        self.p = self.mem.ctypes.data + (-self.mem.ctypes.data) % 16
        self.out = np.zeros((N, T), np.int16)
        self.pending = np.zeros(N, np.int32)
        self.lens = np.full(N, T // 2, np.int32)

    def submit(self, h, rate=True):
        p = self.p
        return [h, 4, p] + ([p if rate else None]) + [p, p, p, None, p, p, p, None]

    def plain_submit(self, h):
        a = self.submit(h)
        return a[:3] + a[4:]

    def relay(self, h, heard=True, slots=2):
        p = self.p
        return [h, p, 8, 64, 12, N, None, 1] + ([p if heard else None, slots]) + [p, p, p, None]

    def plain_relay(self, h):
        a = self.relay(h)
        return a[:8] + a[10:]


def test_create_info_and_destroy(stub):
    h = create_rated(stub, [40] * 36, [0] * 36)                         # 36 entries, all at one rate: fine
    n, depth, maxp, nbytes, want = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    assert stub.afsk_live_tx_info(h, C.byref(n), C.byref(depth), C.byref(maxp), C.byref(nbytes)) == 0
    assert stub.afsk_live_tx_state_bytes_rated(N, 36, DEPTH, MAXP, C.byref(want)) == 0
    assert (n.value, depth.value, maxp.value, nbytes.value) == (N, DEPTH, MAXP, want.value)
    uniform = C.c_int64()
    assert stub.afsk_live_tx_layout(N, DEPTH, MAXP, C.byref(uniform)) == 0
    assert want.value == uniform.value + 512 + 256                      # 288 bytes of table, 192 of entry geometries
    assert stub.afsk_live_tx_destroy(h) == 0
    h = C.c_void_p(77)
    assert stub.afsk_live_tx_create_rated(N, 37, i32([40] * 37)[1], i32([0] * 37)[1], DEPTH, MAXP, C.byref(h)) == \
        _native.E_INVALID_ARG and not h
    assert stub.afsk_live_tx_create_rated(N, 2, i32([40, 6])[1], i32([0, 0])[1], DEPTH, MAXP, C.byref(h)) == \
        _native.E_INVALID_BAUD and not h


def test_a_rated_submit_and_relay_are_two_launches_each(stub):
    h, a = create_rated(stub), Args()
    launches_decoded(stub)
    for rate in (True, False):                                          # a NULL rate_index: entry 0
        assert stub.afsk_live_tx_submit_rated(*a.submit(h, rate)) == 0
        assert launches_decoded(stub) == ["live_tx_order_kernel", "live_tx_submit_rated_kernel"]
    assert stub.afsk_live_tx_submit(*a.plain_submit(h)) == 0            # the plain entry on a rated transmitter
    assert launches_decoded(stub) == ["live_tx_order_kernel", "live_tx_submit_rated_kernel"]
    assert stub.afsk_live_tx_submit_events_rated(*a.relay(h)) == 0
    assert launches_decoded(stub) == ["live_relay_order_kernel", "live_relay_rated_kernel"]
    assert last_kernel(stub)[2] == 1                                    # 8 record places: one block of 16
    assert stub.afsk_live_tx_submit_events(*a.plain_relay(h)) == 0
    assert launches_decoded(stub) == ["live_relay_order_kernel", "live_relay_rated_kernel"]
    # nothing to do: no launch
    args = a.submit(h)
    args[1] = 0
    assert stub.afsk_live_tx_submit_rated(*args) == 0
    args = a.relay(h)
    args[2] = 0
    assert stub.afsk_live_tx_submit_events_rated(*args) == 0
    assert launches_decoded(stub) == []
    # the argument checks of the rated entries
    bad = _native.E_INVALID_ARG
    assert stub.afsk_live_tx_submit_events_rated(*a.relay(h, heard=False)) == bad
    assert "d_rx_bit_frames" in last_error(stub)
    assert stub.afsk_live_tx_submit_events_rated(*a.relay(h, slots=0)) == bad
    args = a.submit(h)
    args[1] = -1
    assert stub.afsk_live_tx_submit_rated(*args) == bad
    args = a.submit(h)
    args[2] = None                                                      # no channels
    assert stub.afsk_live_tx_submit_rated(*args) == bad
    assert launches_decoded(stub) == []
    assert not a.mem.any()
    assert stub.afsk_live_tx_destroy(h) == 0


def test_a_rated_pull_launches_the_rated_tile_kernel(stub):
    h, a = create_rated(stub), Args()
    o, pd, ln = a.out.ctypes.data, a.pending.ctypes.data, a.lens.ctypes.data
    launches_decoded(stub)
    assert stub.afsk_live_tx_pull(h, o, T, T, pd, None) == 0
    assert launches_decoded(stub) == ["live_tx_tile_kernel_rated", "live_tx_commit_kernel"]
    for d_lens in (ln, None):
        assert stub.afsk_live_tx_pull_ragged(h, o, T, T, d_lens, pd, None) == 0
        assert launches_decoded(stub) == ["live_tx_tile_ragged_kernel_rated", "live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_pull(h, None, 0, 0, pd, None) == 0         # nothing to render
    assert launches_decoded(stub) == ["live_tx_commit_kernel"]
    assert stub.afsk_live_tx_reset(h, None, pd, None) == 0
    assert launches_decoded(stub) == ["live_tx_reset_kernel"]
    assert stub.afsk_live_tx_destroy(h) == 0


KINDS = {"uniform_1200": ([40] * N, "live_tx_tile_kernel<0>", "live_tx_tile_ragged_kernel<0>"),
         "uniform_6000": ([8] * N, "live_tx_tile_kernel<1>", "live_tx_tile_ragged_kernel<1>"),
         "mixed": ([40, 8, 160] * (N // 3), "live_tx_tile_kernel_mixed", "live_tx_tile_ragged_kernel_mixed")}


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_other_transmitters_launch_what_they_did_and_refuse_the_rated_entries(stub, kind):
    bfs, tile, tile_ragged = KINDS[kind]
    h, a = create_mixed(stub, bfs), Args()
    o, pd, ln = a.out.ctypes.data, a.pending.ctypes.data, a.lens.ctypes.data
    launches_decoded(stub)
    assert stub.afsk_live_tx_pull(h, o, T, T, pd, None) == 0
    assert launches_decoded(stub) == [tile, "live_tx_commit_kernel"]
    assert stub.afsk_live_tx_pull_ragged(h, o, T, T, ln, pd, None) == 0
    assert launches_decoded(stub) == [tile_ragged, "live_tx_commit_ragged_kernel"]
    assert stub.afsk_live_tx_submit(*a.plain_submit(h)) == 0
    assert launches_decoded(stub) == ["live_tx_order_kernel", "live_tx_submit_kernel"]
    assert stub.afsk_live_tx_submit_events(*a.plain_relay(h)) == 0
    assert launches_decoded(stub) == ["live_relay_order_kernel", "live_relay_kernel"]
    bad = _native.E_INVALID_ARG
    for rate in (True, False):
        assert stub.afsk_live_tx_submit_rated(*a.submit(h, rate)) == bad
        assert "afsk_live_tx_create_rated" in last_error(stub) and "afsk_live_tx_submit" in last_error(stub)
    assert stub.afsk_live_tx_submit_events_rated(*a.relay(h)) == bad
    assert "afsk_live_tx_create_rated" in last_error(stub) and "afsk_live_tx_submit_events" in last_error(stub)
    assert launches_decoded(stub) == []                                 # nothing was launched
    assert not a.mem.any()
    assert stub.afsk_live_tx_destroy(h) == 0


# ------------------------------------------------------------------ the Python layer's ValueErrors (no device needed)

def bare(rated):
    """A LiveTransmitter as far as the checks in front of the device read it (none can be created without one)."""
    tx = object.__new__(live.LiveTransmitter)
    tx.n_channels, tx.rated = 4, rated
    tx.rates = (1200, 300, 1200) if rated else None
    tx.rate_bit_frames = np.asarray([40, 160, 40], np.int32) if rated else None
    tx.rate_ts_cycles = np.asarray([600, 150, 0], np.int32) if rated else None
    tx.bit_frames, tx.ts_cycles = (None, None) if rated else (40, 600)
    return tx


def test_python_rate_lookups_and_refusals():
    tx = bare(True)
    assert tx._rate_index(None, (3,)).tolist() == [0, 0, 0]
    assert tx._rate_index(300, (2,)).tolist() == [1, 1]
    assert tx._rate_index([1200, 300, 1200]).tolist() == [0, 1, 0]      # the first entry at 1200
    assert tx.message_len(3, baud_rate=300) == 160 * (300 + 4 + 42) + 4800
    assert tx.message_len([0, 1], baud_rate=[1200, 300]).tolist() == [40 * 1204 + 4800, 160 * 318 + 4800]
    assert tx.message_len(0) == 40 * 1204 + 4800
    with pytest.raises(ValueError, match=r"\[2400\] are not in the transmitter's table"):
        tx._rate_index([1200, 2400])
    with pytest.raises(ValueError, match="not in the transmitter's table"):
        tx.submit([0, 1], [b"a", b"b"], baud_rate=[1200, 9600])
    with pytest.raises(ValueError, match="not in the transmitter's table"):
        tx.message_len(3, baud_rate=2400)
    with pytest.raises(ValueError, match="3 baud rates for 2 payloads"):
        tx.submit([0, 1], [b"a", b"b"], baud_rate=[1200, 300, 300])
    plain = bare(False)
    with pytest.raises(ValueError, match="needs a rated transmitter"):
        plain.submit([0], [b"a"], baud_rate=1200)
    with pytest.raises(ValueError, match="needs a rated transmitter"):
        plain.message_len(3, baud_rate=1200)
    assert plain.message_len(3) == 40 * (1200 + 4 + 42) + 4800


def test_python_submit_events_rate_refusals():
    ev = live.LiveEvents(np.zeros(4096, np.uint8), 2, 16)
    with pytest.raises(ValueError, match="needs a rated transmitter"):
        bare(False).submit_events(ev, rate="heard")
    with pytest.raises(ValueError, match='None or "heard"'):
        bare(True).submit_events(ev, rate="sent")
    fixed = live.LiveResult(None, None, None, None, None)               # a fixed-rate receiver's: no bit_frames
    ev = live.LiveEvents(np.zeros(4096, np.uint8), 2, 16, result=fixed)
    with pytest.raises(ValueError, match="auto receiver"):
        bare(True).submit_events(ev, rate="heard")
