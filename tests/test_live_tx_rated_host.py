"""Host side of the rated live transmitter (no GPU): the C-ABI declarations, their signature table and the library's
exports, the argument checks of afsk_live_tx_create_rated / afsk_live_tx_state_bytes_rated that return before a device
is needed, the state bytes, the no-device error, and the rated queue model (tests/live_tx_rated_model.py) against
hand-worked cases."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_tx_rated_model as RM
from tests.stub_lib import i32
from tests.test_live_ragged_host import declared_args, header
from tests.test_live_relay_host import hand_buffer

ENTRIES = ("afsk_live_tx_state_bytes_rated", "afsk_live_tx_create_rated", "afsk_live_tx_submit_rated",
           "afsk_live_tx_submit_events_rated")
Q, FULL, LONG, BAD, UNSORTED = (_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUE_FULL, _native.LIVE_TX_TOO_LONG,
                                _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED)
SKIPPED, NONE, BAD_RATE = _native.LIVE_TX_SKIPPED, _native.LIVE_TX_NONE, _native.LIVE_TX_BAD_RATE


def test_header_declares_the_entries_and_the_status_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_TX_RATED_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_TX_RATED_SIGNATURES[name]
        want = declared_args(hdr, name)
        assert res is C.c_int and len(args) == len(want), name
        assert all(a is w or (w is C.c_void_p and issubclass(a, C._Pointer)) for a, w in zip(args, want)), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_tx_submit_events(")
    others = [getattr(_native, t) for t in dir(_native)
              if t.endswith("SIGNATURES") and t != "LIVE_TX_RATED_SIGNATURES"]
    assert len(others) >= 15 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert int(re.search(r"#define AFSK_LIVE_TX_BAD_RATE (\d+)", hdr).group(1)) == BAD_RATE == 6
    assert len({Q, FULL, LONG, BAD, UNSORTED, SKIPPED, NONE, BAD_RATE}) == 8
    # the submit entries are the plain ones with the rate arguments put in
    plain = _native.LIVE_TX_SIGNATURES["afsk_live_tx_submit"][1]
    assert _native.LIVE_TX_RATED_SIGNATURES["afsk_live_tx_submit_rated"][1] == plain[:3] + [C.c_void_p] + plain[3:]
    relay = _native.LIVE_RELAY_SIGNATURES["afsk_live_tx_submit_events"][1]
    assert _native.LIVE_TX_RATED_SIGNATURES["afsk_live_tx_submit_events_rated"][1] == \
        relay[:8] + [C.c_void_p, C.c_int32] + relay[8:]


def test_library_exports_and_binds_the_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_TX_RATED_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


def state_bytes(n, n_rates, depth, maxp):
    out = C.c_int64(-1)
    rc = _native.lib().afsk_live_tx_state_bytes_rated(n, n_rates, depth, maxp, C.byref(out))
    return rc, out.value


def align256(x):
    return (x + 255) // 256 * 256


def test_state_bytes_are_the_uniform_bytes_plus_the_two_aligned_parts():
    for n, k, depth, maxp in ((1, 1, 1, 0), (6, 6, 4, 64), (7, 36, 3, 100), (65537, 3, 5, 16), (33, 32, 1024, 1)):
        rc, got = state_bytes(n, k, depth, maxp)
        assert rc == 0
        assert got == live.tx_layout(n, depth, maxp) + align256(8 * k) + align256(8 * n * depth), (n, k, depth, maxp)
        assert got == live.tx_state_bytes_rated(n, k, depth, maxp) and got % 256 == 0
    assert _native.lib().afsk_live_tx_state_bytes_rated(6, 3, 4, 64, None) == 0           # nothing to write to
    bad = _native.E_INVALID_ARG
    for args in ((0, 3, 4, 64), (6, 0, 4, 64), (6, 37, 4, 64), (6, -1, 4, 64), (6, 3, 0, 64), (6, 3, 1025, 64),
                 (6, 3, 4, -1), (6, 3, 4, 65537)):
        assert state_bytes(*args) == (bad, -1), args


def create(n, bfs, ts, depth=4, maxp=64, n_rates=None, out=True):
    (keep_b, b), (keep_t, t) = i32(bfs if bfs is not None else [0]), i32(ts if ts is not None else [0])
    h = C.c_void_p(1234)
    rc = _native.lib().afsk_live_tx_create_rated(n, len(bfs) if n_rates is None else n_rates,
                                                 b if bfs is not None else None, t if ts is not None else None,
                                                 depth, maxp, C.byref(h) if out else None)
    return rc, h


def test_create_refuses_bad_arguments_before_it_needs_a_device():
    bad, baud = _native.E_INVALID_ARG, _native.E_INVALID_BAUD
    rc, h = create(6, [40], [0], n_rates=0)
    assert rc == bad and not h and "n_rates" in _native.last_error()
    rc, h = create(6, [40] * 37, [0] * 37)
    assert rc == bad and not h and "n_rates" in _native.last_error()
    assert create(6, [40], [0], n_rates=-1)[0] == bad
    for value in (6, 0, 2, 41, -40, 48004):
        rc, h = create(6, [40, value, 160], [10, 10, 10])
        assert rc == baud and not h, value
        assert "multiple of 4" in _native.last_error()
    assert create(6, None, [0], n_rates=1)[0] == bad
    assert create(6, [40], None, n_rates=1)[0] == bad
    assert create(6, [40], [0], out=False)[0] == bad
    assert create(0, [40], [0])[0] == bad
    assert create(6, [40], [0], depth=0)[0] == bad and create(6, [40], [0], depth=1025)[0] == bad
    assert create(6, [40], [0], maxp=-1)[0] == bad and create(6, [40], [0], maxp=65537)[0] == bad
    # the longest message of ONE entry past AFSK_MAX_STREAM_LEN
    assert 40 * (4 + 14 * 65536) + 4800 <= _native.MAX_STREAM_LEN < 2000 * (4 + 14 * 65536) + 4800
    rc, h = create(6, [40, 2000], [0, 0], maxp=65536)
    assert rc == bad and not h and "AFSK_MAX_STREAM_LEN" in _native.last_error()
    # ... and by its training alone
    assert 40 * (2 * 2 ** 24 + 4) + 4800 > _native.MAX_STREAM_LEN
    rc, h = create(6, [40, 40], [0, 2 ** 24], maxp=0)
    assert rc == bad and not h and "AFSK_MAX_STREAM_LEN" in _native.last_error()


def test_create_and_the_rated_submits_need_a_device():
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, h = create(6, [40, 160, 40], [600, 150, 0])                   # (equal bit_frames in two entries are fine)
    assert rc == _native.E_NO_DEVICE and not h
    with pytest.raises(_native.AfskNativeError) as ei:
        live.LiveTransmitter(6, rates=[1200, 300])
    assert ei.value.code == _native.E_NO_DEVICE
    # zeroed host memory stands for a transmitter that is not rated: refused before a device is asked for
    mem = np.zeros(4096, np.uint8)
    p = mem.ctypes.data + (-mem.ctypes.data) % 16
    lib = _native.lib()
    assert lib.afsk_live_tx_submit_rated(p, 2, p, p, p, p, p, None, p, p, p, None) == _native.E_INVALID_ARG
    assert "afsk_live_tx_create_rated" in _native.last_error()
    assert lib.afsk_live_tx_submit_events_rated(p, p, 2, 16, 8, 4, None, 1, p, 2, p, p, p, None) == \
        _native.E_INVALID_ARG
    assert "afsk_live_tx_create_rated" in _native.last_error()
    assert lib.afsk_live_tx_submit_rated(None, 2, p, p, p, p, p, None, p, p, p, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_tx_submit_events_rated(p, p, 2, 16, 8, 4, None, 1, None, 2, p, p, p, None) == \
        _native.E_INVALID_ARG
    assert lib.afsk_live_tx_submit_events_rated(p, p, 2, 16, 8, 4, None, 1, p, 0, p, p, p, None) == \
        _native.E_INVALID_ARG
    assert not mem.any()


def test_python_refuses_a_bad_table_before_it_needs_a_device():
    with pytest.raises(ValueError, match="per-channel baud_rate"):
        live.LiveTransmitter(2, [1200, 300], rates=[1200])
    with pytest.raises(ValueError, match="1 ... 36"):
        live.LiveTransmitter(2, rates=[])
    with pytest.raises(ValueError, match="1 ... 36"):
        live.LiveTransmitter(2, rates=[1200] * 37)
    with pytest.raises(ValueError, match="multiple of 4"):
        live.LiveTransmitter(2, rates=[1200, 7])
    with pytest.raises(ValueError, match="training_time"):
        live.LiveTransmitter(2, rates=[1200, 300], training_time=[0.5, 0.5, 0.5])


# ---------------------------------------------------------------------------------- the model, hand-worked cases

TABLE = [(40, 0), (8, 0), (40, 5)]                                   # 1200 baud, 6000 baud, 1200 baud with training


def ns(entry, plen):
    bf, ts = TABLE[entry]
    return bf * (2 * ts + 4 + 14 * plen) + 4800


def model(n=4, depth=2, maxp=6):
    return RM.LiveTxRatedModel(n, TABLE, depth, maxp)


def test_model_sample_counts_are_the_entrys():
    assert (ns(0, 3), ns(1, 3), ns(2, 3)) == (6640, 5168, 7040)
    m = model()
    assert [m.n_samples(3, e) for e in range(3)] == [6640, 5168, 7040]
    assert [m.entry_of(bf) for bf in (40, 8, 160, 0)] == [0, 1, 3, 3]  # the FIRST entry at 40; none: len(table)


def test_model_queues_back_to_back_at_each_messages_own_rate():
    m = model(depth=3)
    st, start, n = m.submit([1, 1, 1, 0], [b"abc", b"de", b"f", b""], [1, 2, 0, 1])
    assert st.tolist() == [Q, Q, Q, Q]
    assert n.tolist() == [ns(1, 3), ns(2, 2), ns(0, 1), ns(1, 0)]
    assert start.tolist() == [0, ns(1, 3), ns(1, 3) + ns(2, 2), 0]
    assert m.pull(ns(1, 0)).tolist() == [0, 3, 0, 0]                  # channel 0's empty message has ended
    assert m.pull(ns(1, 3) - ns(1, 0)).tolist() == [0, 2, 0, 0]       # ... now channel 1's first
    # None: entry 0 for all
    st, start, n = model().submit([2, 2], [b"abc", b"abc"])
    assert n.tolist() == [ns(0, 3)] * 2 and start.tolist() == [0, ns(0, 3)]


def test_model_refusals_come_in_the_stated_order():
    m = model(n=2, depth=1, maxp=2)
    # unsorted beats everything; a bad channel beats too long, a bad rate and a full queue; too long beats a bad rate;
    # a bad rate beats a full queue
    st, start, n = m.submit([0, 0, 0, 0, 1, 1, 5, 0], [b"a", b"abc", b"abc", b"b", b"a", b"a", b"abc", b"abc"],
                            [0, 9, 0, -1, 3, 2, 9, 9], sort=False)
    assert st.tolist() == [Q, LONG, LONG, BAD_RATE, BAD_RATE, Q, BAD, UNSORTED]
    assert start.tolist() == [0, -1, -1, -1, -1, 0, -1, -1]
    assert n.tolist() == [ns(0, 1), 0, 0, 0, 0, ns(2, 1), 0, 0]
    st, _, _ = m.submit([0, 0], [b"a", b"a"], [0, 3])                  # the queue is full: the bad rate is named first
    assert st.tolist() == [FULL, BAD_RATE]
    assert m.pending().tolist() == [1, 1]


def test_model_relay_at_the_rate_heard():
    rows = [(0, 0, 0, 3, 0),        # slot 0 of channel 0: heard at 8 -> entry 1
            (0, 0, 0, 2, 3),        # the same slot again (a hand-made list): entry 1, behind the first
            (1, 0, 0, 2, 5),        # heard at 160: not in the table
            (1, 0, 0, 7, 7),        # too long, decided in front of the rate
            (2, 0, 1, 2, 14),       # its status is not OK (a TOO_SHORT burst, its rate 0): not relayable
            (2, 0, 0, 2, 16),       # heard 0 with status OK: BAD_RATE
            (3, 0, 0, 1, 18),       # heard at 40: the FIRST entry at 40 (entry 0, no training)
            (9, 0, 0, 1, 19)]       # no such receiver channel: no place in the rate array
    buf = hand_buffer(rows, 10, 40)
    recs = RM.R.parts(buf, 10, 40)[1]
    recs["slot"][6] = 1             # (a view: record 6 is slot 1 of channel 3)
    rx_bf = np.array([[8, 0], [160, 0], [0, 0], [0, 40]], np.int32)
    m = model(depth=2)
    st, start, n, queued = RM.relay_heard(m, buf, 10, 40, 8, 4, rx_bf)
    assert st.tolist() == [Q, Q, BAD_RATE, LONG, SKIPPED, BAD_RATE, Q, SKIPPED, NONE, NONE]
    assert start.tolist() == [0, ns(1, 3), -1, -1, -1, -1, 0, -1, -1, -1]
    assert n.tolist() == [ns(1, 3), ns(1, 2), 0, 0, 0, 0, ns(0, 1), 0, 0, 0]
    assert [(d, e) for d, _, e in queued] == [(0, 1), (0, 1), (1, 3), (1, 3), (2, 3), (3, 0)]
    # a slot outside the array is SKIPPED; a dropped channel too; the map moves channel 3 to 0
    recs["slot"][0] = 2
    st, _, n, queued = RM.relay_heard(model(), buf, 10, 40, 8, 4, rx_bf, channel_map=[-1, 1, 2, 0])
    assert st.tolist() == [SKIPPED, SKIPPED, BAD_RATE, LONG, SKIPPED, BAD_RATE, Q, SKIPPED, NONE, NONE]
    assert [(d, e) for d, _, e in queued] == [(1, 3), (1, 3), (2, 3), (0, 0)]


def test_model_ragged_pull_advances_each_channel_by_its_own_length():
    m = model(n=3, depth=2)
    m.submit([0, 1, 2], [b"a", b"a", b"a"], [1, 1, 1])
    assert m.pull_ragged(6000, [ns(1, 1), ns(1, 1) - 1, -5]).tolist() == [0, 1, 1]
    assert m.pos == [ns(1, 1), ns(1, 1) - 1, 0]
    assert m.pull_ragged(1, [1, 1, 9]).tolist() == [0, 0, 1] and m.pos[2] == 1
