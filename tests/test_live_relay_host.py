"""Host side of the relay submit (no GPU): the C-ABI declarations, their signature table and the library's exports,
``afsk_live_relay_check_map`` on every kind of map, the argument checks of ``afsk_live_tx_submit_events`` that come
before anything of the transmitter is touched, the relay model (tests/live_relay_model.py) against hand-worked cases,
and the no-device error of ``LiveTransmitter.submit_events``."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_events_model as M
from tests import live_relay_model as R
from tests.live_tx_model import LiveTxModel
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_relay_check_map", "afsk_live_tx_submit_events")
Q, FULL, LONG, BAD, UNSORTED = (_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUE_FULL, _native.LIVE_TX_TOO_LONG,
                                _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED)
SKIPPED, NONE = _native.LIVE_TX_SKIPPED, _native.LIVE_TX_NONE


def test_header_declares_the_entries_and_statuses_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_RELAY_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_RELAY_SIGNATURES[name]
        want = declared_args(hdr, name)
        assert res is C.c_int and len(args) == len(want), name
        assert all(a is w or (w is C.c_void_p and issubclass(a, C._Pointer)) for a, w in zip(args, want)), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_pack(")
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_tx_submit(")
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_RELAY_SIGNATURES"]
    assert len(others) >= 14 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert int(re.search(r"#define AFSK_LIVE_TX_SKIPPED (\d+)", hdr).group(1)) == SKIPPED == 5
    assert int(re.search(r"#define AFSK_LIVE_TX_NONE \((-\d+)\)", hdr).group(1)) == NONE == -1
    assert len({Q, FULL, LONG, BAD, UNSORTED, SKIPPED, NONE}) == 7


def test_library_exports_and_binds_both_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_RELAY_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


# -------------------------------------------------------------------------------------- afsk_live_relay_check_map

def check_map(values, n_tx, n_rx=None):
    if values is None:
        return _native.lib().afsk_live_relay_check_map(None, n_rx, n_tx)
    v = np.ascontiguousarray(values, np.int32)
    ptr = v.ctypes.data_as(C.POINTER(C.c_int32))
    return _native.lib().afsk_live_relay_check_map(ptr, v.size if n_rx is None else n_rx, n_tx)


def test_check_map_accepts_what_gives_every_destination_one_source():
    assert check_map(None, 4, n_rx=4) == 0 and check_map(None, 1, n_rx=65537) == 0        # NULL: the identity
    assert check_map(np.arange(70), 70) == 0
    assert check_map(np.random.default_rng(1).permutation(75)[:70], 75) == 0
    assert check_map([3, -1, 0, -1, -1, 2], 4) == 0                                        # drops
    assert check_map([-1, -1, -7, -1], 4) == 0                                             # equal negative values
    assert check_map([4, 4, 99, 99, 2 ** 31 - 1, 2 ** 31 - 1], 4) == 0                     # equal out-of-range values
    assert check_map([0, 4, 1, 4, -2, -2, 3], 4) == 0
    assert check_map([0], 1) == 0 and check_map([-1], 1) == 0 and check_map([1], 1) == 0   # n = 1
    assert check_map([5], 9) == 0


def test_check_map_refuses_two_sources_of_one_destination_and_names_them():
    bad = _native.E_INVALID_ARG
    assert check_map([0, 1, 2, 1], 4) == bad
    msg = _native.last_error()
    assert re.search(r"\b1 and 3\b", msg) and "transmitter channel 1" in msg, msg
    assert check_map([3, 3], 4) == bad
    assert re.search(r"\b0 and 1\b", _native.last_error()) and "transmitter channel 3" in _native.last_error()
    assert check_map([3, 3], 3) == 0                                                       # (3 is out of range there)
    assert check_map([7, -1, 2, 5, 2, 7], 7) == bad                                        # 7 is out of range, 2 is not
    assert re.search(r"\b2 and 4\b", _native.last_error()) and "transmitter channel 2" in _native.last_error()
    with pytest.raises(_native.AfskNativeError) as ei:
        _native.check(check_map([0, 0], 1))
    assert ei.value.code == bad and "0 and 1" in str(ei.value)


def test_check_map_at_65537_channels():
    n = 65537
    assert check_map(np.arange(n), n) == 0
    assert check_map(np.arange(n)[::-1], n) == 0
    assert check_map(np.random.default_rng(2).permutation(n), n) == 0
    v = np.arange(n)
    v[n - 1] = 0
    assert check_map(v, n) == _native.E_INVALID_ARG
    assert re.search(r"\b0 and 65536\b", _native.last_error()) and "transmitter channel 0" in _native.last_error()
    v[n - 1] = n                                                                           # past the transmitter
    assert check_map(v, n) == 0
    v[7] = v[n - 2] = -1
    assert check_map(v, n) == 0


def test_check_map_refuses_bad_sizes():
    for n_rx, n_tx in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert check_map([0, 1, 2, 3], n_tx, n_rx=n_rx) == _native.E_INVALID_ARG, (n_rx, n_tx)
        assert check_map(None, n_tx, n_rx=n_rx) == _native.E_INVALID_ARG, (n_rx, n_tx)


# ----------------------------------------------------------- afsk_live_tx_submit_events: the checks in front of tx

def test_submit_events_refuses_bad_arguments_before_it_touches_the_transmitter():
    """Every refusal comes before anything of the transmitter, the events or the outputs is read: the pointers here
    point at zeroed host memory that no accepted call may ever be given."""
    lib = _native.lib()
    mem = np.zeros(4096, np.uint8)
    p = mem.ctypes.data + (-mem.ctypes.data) % 16
    good = dict(tx=p, events=p, max_events=4, max_bytes=64, out_stride=12, n_rx=4, map=None, skip=1, st=p, start=p,
                ns=p, stream=None)
    refusals = [("tx", None), ("events", None), ("st", None), ("start", None), ("ns", None), ("max_events", -1),
                ("max_bytes", -1), ("out_stride", -1), ("n_rx", 0), ("n_rx", -5), ("skip", 4), ("skip", 8 | 1),
                ("skip", -1), ("events", p + 8), ("events", p + 1)]
    for key, value in refusals:
        args = dict(good, **{key: value})
        assert lib.afsk_live_tx_submit_events(*args.values()) == _native.E_INVALID_ARG, (key, value)
        assert _native.last_error(), key
    assert "16-byte aligned" in _native.last_error()
    for skip in (0, 1, 2, 3):                                    # max_events == 0: AFSK_OK, nothing launched or read
        assert lib.afsk_live_tx_submit_events(*dict(good, max_events=0, skip=skip).values()) == 0
    assert not mem.any()


# ---------------------------------------------------------------------------------- the model, hand-worked cases

def hand_buffer(rows, max_events, max_bytes, payload=None, stored=None, count=None):
    """An events buffer of the records ``rows`` -- (channel, flags, status, nbytes, payload_offset) each -- over a
    payload part holding the bytes 1, 2, 3, ... (byte k is k + 1) unless ``payload`` is given."""
    recs = np.zeros(len(rows), M.EVENT)
    for i, (ch, fl, st, nb, off) in enumerate(rows):
        recs[i] = (ch, 0, 2048 * i, 2048, fl, st, nb, 8 * nb, 0, 0, off)
    pay = bytes((k + 1) & 0xFF for k in range(max_bytes)) if payload is None else payload
    n = len(rows) if stored is None else stored
    h = np.array([(n if count is None else count, n, len(pay), len(pay), 0)], M.HEADER)
    return M.buffer(h, recs, pay, max_events, max_bytes)


def tx_model(n=4, depth=2, max_payload=6):
    return LiveTxModel(n, 40, 0, depth, max_payload)


def ns40(plen):
    return 40 * (4 + 14 * plen) + 4800


def test_model_reaches_every_status_on_a_hand_worked_list():
    rows = [(0, 0, 0, 3, 0),        # queued at 0
            (0, 0, 0, 7, 3),        # 7 bytes > max_payload_len 6
            (0, 0, 0, 2, 10),       # queued behind the first
            (0, 0, 0, 1, 12),       # the third good record of the run into depth 2
            (1, 1, 0, 2, 13),       # OPEN_END
            (1, 2, 0, 2, 15),       # OVERFLOW
            (2, 0, 2, 2, 17),       # status NO_DATA
            (2, 0, 0, 0, 19),       # no bytes
            (2, 0, 0, 9, 19),       # a truncated streaming row: 9 > out_stride 8
            (3, 0, 0, 2, -1),       # its payload did not fit the buffer
            (7, 0, 0, 2, 28)]       # no such transmitter channel
    buf = hand_buffer(rows, 12, 40)
    st, start, ns, queued = R.relay(tx_model(), buf, 12, 40, 8, 8)
    assert st.tolist() == [Q, LONG, Q, FULL, SKIPPED, SKIPPED, SKIPPED, SKIPPED, SKIPPED, SKIPPED, BAD, NONE]
    assert start.tolist() == [0, -1, ns40(3), -1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert ns.tolist() == [ns40(3), 0, ns40(2), 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert ns40(3) == 6640 and ns40(2) == 6080
    assert queued == [(0, bytes([1, 2, 3])), (0, bytes(range(4, 11))), (0, bytes([11, 12])), (0, bytes([13]))]
    # skip_flags = 0 relays the OPEN_END burst; OVERFLOW is never relayed
    st, start, ns, queued = R.relay(tx_model(), buf, 12, 40, 8, 8, skip_flags=0)
    assert st.tolist()[4:6] == [Q, SKIPPED] and start[4] == 0 and ns[4] == ns40(2)
    assert (1, bytes([14, 15])) in queued
    st, _, _, _ = R.relay(tx_model(), buf, 12, 40, 8, 8, skip_flags=R.OPEN_END | R.OVERFLOW)
    assert st.tolist()[4:6] == [SKIPPED, SKIPPED]


def test_model_stored_is_clamped_and_the_rest_is_none():
    rows = [(0, 0, 0, 1, 0), (1, 0, 0, 1, 1), (2, 0, 0, 1, 2)]
    for stored, want in ((3, [Q, Q, Q, NONE, NONE]), (2, [Q, Q, NONE, NONE, NONE]), (0, [NONE] * 5),
                         (-4, [NONE] * 5), (99, [Q, Q, Q, SKIPPED, SKIPPED])):
        # (record places past the list hold the buffer's fill, 0x5a in every byte: a channel above its predecessor's,
        # so the list stays sorted, and flags with OVERFLOW set, so the place is not relayable)
        buf = hand_buffer(rows, 5, 16, stored=stored)
        st, start, ns, _ = R.relay(tx_model(), buf, 5, 16, 8, 4)
        assert st.tolist() == want, stored
        assert (start[st != Q] == -1).all() and (ns[st != Q] == 0).all()


def test_model_unsorted_from_the_first_descending_record_on():
    rows = [(0, 0, 0, 1, 0), (1, 0, 0, 1, 1), (1, 0, 0, 1, 2), (0, 0, 0, 1, 3), (2, 0, 0, 1, 4), (3, 2, 5, 0, -1)]
    st, start, ns, queued = R.relay(tx_model(), hand_buffer(rows, 8, 16), 8, 16, 8, 4)
    assert st.tolist() == [Q, Q, Q, UNSORTED, UNSORTED, UNSORTED, NONE, NONE]
    assert start.tolist() == [0, 0, ns40(1), -1, -1, -1, -1, -1]
    assert [d for d, _ in queued] == [0, 1, 1]
    rows = [(3, 0, 0, 1, 0), (2, 0, 0, 1, 1)]
    assert R.relay(tx_model(), hand_buffer(rows, 2, 16), 2, 16, 8, 4)[0].tolist() == [Q, UNSORTED]


def test_model_payload_range_must_lie_inside_max_bytes():
    rows = [(0, 0, 0, 4, 12),       # ends at max_bytes exactly
            (1, 0, 0, 4, 13),       # crosses it
            (2, 0, 0, 1, 16),       # starts at it
            (3, 0, 0, 2, 2 ** 31 - 1)]
    st, _, _, queued = R.relay(tx_model(), hand_buffer(rows, 4, 16), 4, 16, 8, 4)
    assert st.tolist() == [Q, SKIPPED, SKIPPED, SKIPPED]
    assert queued == [(0, bytes([13, 14, 15, 16]))]


def test_model_maps_drops_and_refuses_channels():
    rows = [(0, 0, 0, 1, 0), (1, 0, 0, 1, 1), (2, 0, 0, 1, 2), (3, 0, 0, 1, 3), (3, 0, 0, 1, 4), (5, 0, 0, 1, 5),
            (6, 1, 0, 1, 6)]
    cmap = [2, -1, 9, 0]
    st, start, ns, queued = R.relay(tx_model(), hand_buffer(rows, 7, 16), 7, 16, 8, 4, channel_map=cmap)
    # 0 -> 2; 1 dropped; 2 -> 9: no such transmitter channel; 3 -> 0 twice; 5 is no receiver channel; 6 is not
    # relayable, which is decided first
    assert st.tolist() == [Q, SKIPPED, BAD, Q, Q, BAD, SKIPPED]
    assert start.tolist() == [0, -1, -1, 0, ns40(1), -1, -1]
    assert queued == [(2, bytes([1])), (0, bytes([4])), (0, bytes([5]))]
    # without a map the record's channel is the destination, whatever the receiver's channel count
    st, _, _, queued = R.relay(tx_model(n=6), hand_buffer(rows, 7, 16), 7, 16, 8, 4)
    assert st.tolist() == [Q, Q, Q, Q, Q, Q, SKIPPED] and [d for d, _ in queued] == [0, 1, 2, 3, 3, 5]


def test_model_queues_behind_what_the_transmitter_already_holds():
    m = tx_model(depth=3)
    m.submit([1], [b"abc"])
    m.pull(1000)
    rows = [(1, 0, 0, 2, 0), (1, 0, 0, 2, 2), (1, 0, 0, 2, 4), (2, 0, 0, 2, 6)]
    st, start, ns, _ = R.relay(m, hand_buffer(rows, 4, 16), 4, 16, 8, 4)
    assert st.tolist() == [Q, Q, FULL, Q]
    assert start.tolist() == [ns40(3), ns40(3) + ns40(2), -1, 1000]      # behind the message on air; idle: at pos
    assert m.pending().tolist() == [0, 3, 1, 0]


# ------------------------------------------------------------------------------------------------ without a device

def test_submit_events_needs_a_device():
    """Without a GPU the relay submit raises the package's no-device error; there is no CPU stand-in."""
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible")
    tx = object.__new__(live.LiveTransmitter)                    # (no transmitter can be created without a device)
    ev = live.LiveEvents(hand_buffer([(0, 0, 0, 1, 0)], 2, 16), 2, 16)
    with pytest.raises(_native.AfskNativeError) as ei:
        tx.submit_events(ev)
    assert ei.value.code == _native.E_NO_DEVICE and "no HIP device" in str(ei.value)
    # the C entry: its argument checks come first, then the device
    mem = np.zeros(4096, np.uint8)
    p = mem.ctypes.data + (-mem.ctypes.data) % 16
    assert _native.lib().afsk_live_tx_submit_events(p, p, 2, 16, 8, 4, None, 1, p, p, p, None) == _native.E_NO_DEVICE
    assert _native.lib().afsk_live_tx_submit_events(p, p, -2, 16, 8, 4, None, 1, p, p, p, None) == _native.E_INVALID_ARG
