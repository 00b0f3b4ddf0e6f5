"""Host side of the live transmitter (no GPU): the C-ABI declarations, statuses and exports, afsk_live_tx_layout
against a closed form and its argument checks, the Python-side baud rule, the queue model (tests/live_tx_model.py)
against hand-worked cases and against Transmitter's own message lengths, and the no-device error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from tests.live_tx_model import LiveTxModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_ENTRIES = ("afsk_live_tx_layout", "afsk_live_tx_create", "afsk_live_tx_info", "afsk_live_tx_submit",
              "afsk_live_tx_pull", "afsk_live_tx_reset", "afsk_live_tx_destroy")
Q, FULL, LONG, BAD, UNSORTED = (_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUE_FULL, _native.LIVE_TX_TOO_LONG,
                                _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED)


def test_header_declares_live_tx_entries():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    assert "typedef struct afsk_live_tx afsk_live_tx;" in hdr
    for name in TX_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.LIVE_TX_SIGNATURES) == set(TX_ENTRIES)
    for other in (_native.SIGNATURES, _native.SPLIT_SIGNATURES, _native.LIVE_SIGNATURES):
        assert not set(_native.LIVE_TX_SIGNATURES) & set(other)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    for name, value in (("QUEUED", Q), ("QUEUE_FULL", FULL), ("TOO_LONG", LONG), ("BAD_CHANNEL", BAD),
                        ("UNSORTED", UNSORTED)):
        assert int(re.search(r"#define AFSK_LIVE_TX_%s (\d+)" % name, hdr).group(1)) == value, name
    assert len({Q, FULL, LONG, BAD, UNSORTED}) == 5


def test_library_exports_live_tx_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in TX_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2        # binds all four tables


def a256(x):
    return -(-x // 256) * 256


def closed_form(n, depth, max_payload):
    return a256(32 * n) + a256(16 * n * depth) + a256(n * depth * max_payload) + 256


def c_layout(n, depth, max_payload):
    nbytes = C.c_int64(-7)
    rc = _native.lib().afsk_live_tx_layout(n, depth, max_payload, C.byref(nbytes))
    return rc, int(nbytes.value)


@pytest.mark.parametrize("n", [1, 3, 64, 4096, 65536])
def test_layout_closed_form(n):
    for depth in (1, 2, 4, 7, 64, 1024):
        for mp in (0, 1, 64, 255, 256, 1000, 65536):
            rc, nbytes = c_layout(n, depth, mp)
            assert rc == 0, _native.last_error()
            assert nbytes == closed_form(n, depth, mp), (depth, mp)
            assert live.tx_layout(n, depth, mp) == nbytes


@pytest.mark.parametrize("args", [(0, 4, 256), (-1, 4, 256), (4, 0, 256), (4, -2, 256), (4, 1025, 256),
                                  (4, 4, -1), (4, 4, 65537), (1 << 22, 1024, 0)])
def test_layout_refuses_bad_arguments(args):
    rc, nbytes = c_layout(*args)
    assert rc == _native.E_INVALID_ARG and nbytes == -7
    with pytest.raises(_native.AfskNativeError) as ei:
        live.tx_layout(*args)
    assert ei.value.code == _native.E_INVALID_ARG


def test_baud_rule():
    for baud, bf in ((300, 160), (1200, 40), (2400, 20), (12000, 4), (1000, 48), (10, 4800), (1, 48000)):
        assert live.tx_bit_frames(baud) == bf
    for baud in (4800, 8000, 7, 0, -1200, 96000, 1200.5, 48000):
        with pytest.raises(ValueError):
            live.tx_bit_frames(baud)


def test_model_lengths_are_the_transmitters():
    for baud in (300, 1200, 2400, 12000):
        for tt in (0.5, 0.1, 0.0, -1.0):
            t = afskmodem.Transmitter(baud, tt)
            m = LiveTxModel(1, t.bit_frames, t.ts_cycles, 4, 64)
            for p in (b"", b"x", b"Hello World!", bytes(range(64))):
                assert m.n_samples(len(p)) == len(t.wav_samples(p)), (baud, tt, p)


def test_model_hand_worked_queue():
    # 1200 baud, no training: a message of p bytes is 40 * (4 + 14 p) + 4800 samples: 4960 for 0 bytes, 5520 for 1
    m = LiveTxModel(2, 40, 0, 2, 256)
    st, s, n = m.submit([0, 0, 0, 1], [b"", b"a", b"bb", b"x" * 257])
    assert st.tolist() == [Q, Q, FULL, LONG]
    assert s.tolist() == [0, 4960, -1, -1] and n.tolist() == [4960, 5520, 0, 0]
    assert m.pull(1000).tolist() == [2, 0]
    st, s, _ = m.submit([1], ["z"])                        # an idle channel: the next sample pulled
    assert st.tolist() == [Q] and s.tolist() == [1000]
    assert m.pull(3959).tolist() == [2, 1]                 # pos 4959: the first message has one sample left
    assert m.pull(1).tolist() == [1, 1]                    # pos 4960: retired
    st, s, _ = m.submit([0, 2, -1, 0], [b"", b"", b"", b""])
    assert st.tolist() == [Q, BAD, BAD, FULL]              # ch 0 holds 2 again; rejected ones take no entry
    assert s.tolist() == [4960 + 5520, -1, -1, -1]         # back to back, no gap
    assert m.pull(20000).tolist() == [0, 0]                # pos 24960: everything ended
    st, s, _ = m.submit([0], [b""])
    assert s.tolist() == [24960]                           # idle again: starts at pos, not at the old end


def test_model_rejections_leave_later_starts_unchanged():
    m = LiveTxModel(1, 40, 0, 3, 4)
    st, s, _ = m.submit([0] * 5, [b"", b"toolong", b"", b"", b""])
    assert st.tolist() == [Q, LONG, Q, Q, FULL]
    assert s.tolist() == [0, -1, 4960, 9920, -1]


def test_model_sort_and_unsorted_rule():
    m = LiveTxModel(3, 40, 0, 4, 16)
    st, s, _ = m.submit([2, 0, 2, 0], [b"", b"", b"", b""])          # the Python layer sorts stably
    assert st.tolist() == [Q] * 4 and s.tolist() == [0, 0, 4960, 4960]
    m = LiveTxModel(3, 40, 0, 4, 16)
    st, s, _ = m.submit([0, 1, 1, 0, 2], [b""] * 5, sort=False)       # the C rule: unsorted from index 3 on
    assert st.tolist() == [Q, Q, Q, UNSORTED, UNSORTED]
    assert s.tolist() == [0, 0, 4960, -1, -1]


def test_model_reset_and_expected_samples():
    t = afskmodem.Transmitter(1200, 0.0)
    m = LiveTxModel(2, 40, 0, 4, 16, wav=t.wav_samples)
    m.submit([0, 0, 1], [b"a", b"b", b"c"])
    got = np.concatenate([m.expected(7000), (m.pull(7000), m.expected(7000))[1]], axis=1)
    m.pull(7000)
    want0 = np.concatenate([t.wav_samples(b"a"), t.wav_samples(b"b")])
    assert (got[0, : len(want0)] == want0).all() and not got[0, len(want0):].any()
    w1 = t.wav_samples(b"c")
    assert (got[1, : len(w1)] == w1).all() and not got[1, len(w1):].any()
    m.submit([1], [b"d"])                                   # starts at 14000 on channel 1
    m.pull(100)
    m.reset([False, True])                                  # mid-message: dropped, stream restarts at 0
    assert m.pending().tolist() == [0, 0] and m.pos == [14100, 0]
    assert not m.expected(6000)[1].any()
    st, s, _ = m.submit([1], [b"e"])
    assert s.tolist() == [0]


def test_live_transmitter_needs_a_device():
    """Without a GPU the live transmitter raises the package's no-device error; there is no CPU stand-in."""
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_native.AfskNativeError) as ei:
        afskmodem.LiveTransmitter(4, 1200)
    assert ei.value.code == _native.E_NO_DEVICE and "no HIP device" in str(ei.value)
    with pytest.raises(_native.AfskNativeError) as ei:
        afskmodem.Transmitter(1200).live(4)
    assert ei.value.code == _native.E_NO_DEVICE
    h = C.c_void_p()
    assert _native.lib().afsk_live_tx_create(4, 40, 300, 4, 256, C.byref(h)) == _native.E_NO_DEVICE
    assert not h
    for bf in (0, 6, 10, 41, 48004, -40):                   # the baud check comes before the device
        assert _native.lib().afsk_live_tx_create(4, bf, 0, 4, 256, C.byref(h)) == _native.E_INVALID_BAUD, bf
    with pytest.raises(ValueError):
        afskmodem.Transmitter(4800).live(4)
    with pytest.raises(ValueError):
        afskmodem.LiveTransmitter(0, 1200)
