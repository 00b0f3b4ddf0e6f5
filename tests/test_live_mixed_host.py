"""Host side of the live objects with a rate per channel (no GPU): the C-ABI declarations and their signature table,
the argument checks of afsk_live_create_mixed / afsk_live_tx_create_mixed that return before any device is needed,
afsk_live_tx_state_bytes_mixed against a closed form, the Python constructors' checks, and the no-device error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from tests.stub_lib import arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_ENTRIES = ("afsk_live_create_mixed", "afsk_live_tx_create_mixed", "afsk_live_tx_state_bytes_mixed")


def test_header_declares_mixed_entries_in_their_own_table():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    for name in MIXED_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
        assert not re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.LIVE_MIXED_SIGNATURES) == set(MIXED_ENTRIES)
    for other in (_native.SIGNATURES, _native.SPLIT_SIGNATURES, _native.LIVE_SIGNATURES, _native.LIVE_TX_SIGNATURES):
        assert not set(MIXED_ENTRIES) & set(other)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_library_exports_mixed_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in MIXED_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2


def a256(x):
    return -(-x // 256) * 256


def tx_closed_form(n, depth, maxp):
    return a256(32 * n) + a256(16 * n * depth) + a256(n * depth * maxp) + 256 + a256(8 * n)


@pytest.mark.parametrize("n", [1, 3, 31, 33, 4096, 65536])
def test_tx_state_bytes_mixed(n):
    for depth, maxp in ((1, 0), (4, 256), (7, 13), (64, 1000), (1024, 1)):
        got, base = C.c_int64(-7), C.c_int64(-7)
        assert _native.lib().afsk_live_tx_state_bytes_mixed(n, depth, maxp, C.byref(got)) == 0, _native.last_error()
        assert _native.lib().afsk_live_tx_layout(n, depth, maxp, C.byref(base)) == 0
        assert got.value == tx_closed_form(n, depth, maxp)
        assert got.value == base.value + a256(8 * n)           # the layout, then int32 [n, 2] of per-channel geometry
        assert live.tx_state_bytes_mixed(n, depth, maxp) == got.value


@pytest.mark.parametrize("args", [(0, 4, 256), (-1, 4, 256), (4, 0, 256), (4, 1025, 256), (4, 4, -1),
                                  (4, 4, 65537), (1 << 30, 4, 256)])
def test_tx_state_bytes_mixed_refuses_what_the_layout_refuses(args):
    got = C.c_int64(-7)
    assert _native.lib().afsk_live_tx_state_bytes_mixed(*args, C.byref(got)) == _native.E_INVALID_ARG
    assert got.value == -7
    with pytest.raises(_native.AfskNativeError):
        live.tx_state_bytes_mixed(*args)


@pytest.mark.parametrize("bad", [0, 6, 10, 41, 2048, -40])
def test_rx_create_mixed_refuses_a_bad_rate_in_any_channel(bad):
    for where in (0, 2, 4):
        a, p = arr([40, 160, 80, 20, 40])
        a[where] = bad
        h = C.c_void_p(1234)
        assert _native.lib().afsk_live_create_mixed(5, p, 18000, 14000, 96000, 8192, C.byref(h)) \
            == _native.E_INVALID_BAUD, (bad, where)
        assert not h


def test_rx_create_mixed_argument_checks():
    h = C.c_void_p(1234)
    a, p = arr([40, 160])
    assert _native.lib().afsk_live_create_mixed(2, None, 18000, 14000, 96000, 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert not h
    for n in (0, -1):
        assert _native.lib().afsk_live_create_mixed(n, p, 18000, 14000, 96000, 8192, C.byref(h)) \
            == _native.E_INVALID_ARG
    assert _native.lib().afsk_live_create_mixed(2, p, 18000, 14000, 96000, 8192, None) == _native.E_INVALID_ARG
    # the capacities are afsk_live_create's (a burst longer than AFSK_MAX_STREAM_LEN is never stored)
    for mb, mc in ((4095, 8192), (_native.MAX_STREAM_LEN + 1, 8192), (96000, 0), (96000, _native.MAX_STREAM_LEN + 1)):
        assert _native.lib().afsk_live_create_mixed(2, p, 18000, 14000, mb, mc, C.byref(h)) == _native.E_INVALID_ARG
        assert not h


@pytest.mark.parametrize("bad", [0, 6, 10, 41, 48004, -40])
def test_tx_create_mixed_refuses_a_bad_rate_in_any_channel(bad):
    for where in (0, 3):
        a, p = arr([40, 160, 4, 2000])
        t, tp = arr([300, 75, 0, 12])
        a[where] = bad
        h = C.c_void_p(1234)
        assert _native.lib().afsk_live_tx_create_mixed(4, p, tp, 4, 256, C.byref(h)) == _native.E_INVALID_BAUD
        assert not h


def test_tx_create_mixed_argument_checks():
    h = C.c_void_p(1234)
    a, p = arr([40, 160])
    t, tp = arr([300, 75])
    assert _native.lib().afsk_live_tx_create_mixed(2, None, tp, 4, 256, C.byref(h)) == _native.E_INVALID_ARG
    assert _native.lib().afsk_live_tx_create_mixed(2, p, None, 4, 256, C.byref(h)) == _native.E_INVALID_ARG
    assert not h
    for n in (0, -1):
        assert _native.lib().afsk_live_tx_create_mixed(n, p, tp, 4, 256, C.byref(h)) == _native.E_INVALID_ARG
    assert _native.lib().afsk_live_tx_create_mixed(2, p, tp, 4, 256, None) == _native.E_INVALID_ARG
    for depth, maxp in ((0, 256), (1025, 256), (4, -1), (4, 65537)):
        assert _native.lib().afsk_live_tx_create_mixed(2, p, tp, depth, maxp, C.byref(h)) == _native.E_INVALID_ARG


def test_tx_create_mixed_checks_the_longest_message_per_channel():
    # channel 1 alone is too long: bf 48000 * (2 * 0 + 4 + 14 * maxp) + 4800 > AFSK_MAX_STREAM_LEN
    maxp = (_native.MAX_STREAM_LEN - 4800) // (48000 * 14)            # channel 1 just fits at this payload
    for bf1, ok in ((48000, True), (48000, False)):
        m = maxp if ok else maxp + 1
        a, p = arr([40, bf1, 4])
        t, tp = arr([300, 0, 5000])
        h = C.c_void_p()
        rc = _native.lib().afsk_live_tx_create_mixed(3, p, tp, 4, m, C.byref(h))
        if ok:
            # every channel fits: the device is the next thing needed
            assert rc in (_native.E_NO_DEVICE, _native.OK)
            if rc == _native.OK:
                _native.lib().afsk_live_tx_destroy(h)
        else:
            assert rc == _native.E_INVALID_ARG and "AFSK_MAX_STREAM_LEN" in _native.last_error()
    # a long training run makes one channel too long at a small payload
    a, p = arr([40, 2000])
    t, tp = arr([0, _native.MAX_STREAM_LEN // 4000 + 1])
    h = C.c_void_p()
    assert _native.lib().afsk_live_tx_create_mixed(2, p, tp, 4, 0, C.byref(h)) == _native.E_INVALID_ARG


def test_from_receivers_refuses_differing_thresholds():
    with pytest.raises(ValueError, match="thresholds"):
        live.LiveReceiver.from_receivers([afskmodem.Receiver(1200), afskmodem.Receiver(300, 18000, 12000)])
    with pytest.raises(ValueError, match="thresholds"):
        live.LiveReceiver.from_receivers([afskmodem.Receiver(1200, 17000), afskmodem.Receiver(1200)])
    with pytest.raises(ValueError):
        live.LiveReceiver.from_receivers([])
    with pytest.raises(ValueError):
        live.LiveTransmitter.from_transmitters([])


def test_rate_arrays_of_the_wrong_length():
    for rates in ([40, 80, 160], [40] * 5, [[40, 80], [40, 80]], np.full(3, 40)):
        with pytest.raises(ValueError):
            live.LiveReceiver(4, rates)
    for bauds in ([1200, 300], [1200] * 5, np.full(3, 1200)):
        with pytest.raises(ValueError):
            live.LiveTransmitter(4, bauds)
    with pytest.raises(ValueError):
        live.LiveTransmitter(4, 1200, [0.5, 0.1])
    with pytest.raises(ValueError):                         # 4800 baud stays refused, in any channel
        live.LiveTransmitter(3, [1200, 4800, 300])


def test_rate_arrays_reach_the_no_device_error():
    """A per-channel rate array is accepted up to the device: without a GPU the package's no-device error, never a
    TypeError; the C entries refuse nothing else first."""
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible")
    cases = [lambda: live.LiveReceiver(4, [40, 160, 80, 20]),
             lambda: live.LiveReceiver(4, np.array([40, 160, 80, 20])),
             lambda: live.LiveReceiver(4, (40, 40, 40, 40)),
             lambda: live.LiveReceiver.from_receivers([afskmodem.Receiver(b) for b in (1200, 300, 2400, 600)]),
             lambda: live.LiveTransmitter(4, [1200, 300, 2400, 600]),
             lambda: live.LiveTransmitter(4, 1200, [0.5, 0.1, 0.0, 1.0]),
             lambda: live.LiveTransmitter(3, np.array([1200, 300, 12000]), np.array([0.5, 0.25, 0.1])),
             lambda: live.LiveTransmitter.from_transmitters([afskmodem.Transmitter(b) for b in (1200, 300)])]
    for make in cases:
        with pytest.raises(_native.AfskNativeError) as ei:
            make()
        assert ei.value.code == _native.E_NO_DEVICE
    h = C.c_void_p()
    a, p = arr([40, 160, 80, 20])
    t, tp = arr([300, 75, 150, 0])
    assert _native.lib().afsk_live_create_mixed(4, p, 18000, 14000, 96000, 8192, C.byref(h)) == _native.E_NO_DEVICE
    assert _native.lib().afsk_live_tx_create_mixed(4, p, tp, 4, 256, C.byref(h)) == _native.E_NO_DEVICE
    assert not h


def test_message_len_uses_each_channels_geometry():
    """message_len on a mixed transmitter (built without a device: only the host-side fields are read)."""
    tx = object.__new__(live.LiveTransmitter)
    tx.n_channels = 3
    tx.bit_frames = tx.ts_cycles = None
    tx.channel_bit_frames = np.array([40, 160, 4], np.int32)
    tx.channel_ts_cycles = np.array([300, 75, -1], np.int32)
    want = [afskmodem.Transmitter(b, t).wav_samples(b"ab").size for b, t in ((1200, 0.5), (300, 0.5), (12000, 0.0))]
    assert tx.message_len(2, channels=[0, 1, 2]).tolist() == want
    assert tx.message_len(2).tolist() == want
    assert tx.message_len([2, 0], channels=[1, 1]).tolist() == [want[1], want[1] - 160 * 28]
    assert tx.message_len(2, channels=2) == want[2]
    with pytest.raises(ValueError):
        tx.message_len(2, channels=3)
