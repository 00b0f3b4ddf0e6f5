"""Host side of the live receivers with a threshold pair per channel (no GPU): the C-ABI declarations and their
signature table, the argument checks of afsk_live_create_thresholds / afsk_live_create_stream_thresholds that return
before any device is needed (the stored receiver's cap on distinct amp_end values among them), the Python
constructor's per-channel arguments and attributes, and the stored receiver's squelch classes (the slot lists its
demod launches walk) as a partition of the slots."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, live
from tests.stub_lib import arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD_ENTRIES = ("afsk_live_create_thresholds", "afsk_live_create_stream_thresholds")
STORED = ("afsk_live_create_thresholds", 96000)
STREAM = ("afsk_live_create_stream_thresholds", 256)


def create(kind, bf, start, end, cap=None, chunk=8192, n=None):
    name, default_cap = kind
    (b, bp), (s, sp), (e, ep) = arr(bf), arr(start), arr(end)
    h = C.c_void_p(1234)
    rc = getattr(_native.lib(), name)(len(b) if n is None else n, bp, sp, ep, default_cap if cap is None else cap,
                                      chunk, C.byref(h))
    if rc == _native.OK:
        _native.lib().afsk_live_destroy(h)
    else:
        assert not h
    return rc


def test_header_declares_threshold_entries_in_their_own_table():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    for name in THRESHOLD_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
        assert not re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.LIVE_THRESHOLD_SIGNATURES) == set(THRESHOLD_ENTRIES)
    assert int(re.search(r"#define AFSK_LIVE_MAX_SQUELCH_CLASSES (\d+)", hdr).group(1)) == 16 \
        == _native.LIVE_MAX_SQUELCH_CLASSES
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    # the older tables keep their entries
    assert set(_native.LIVE_SIGNATURES) == {"afsk_live_layout", "afsk_live_create", "afsk_live_info", "afsk_live_push",
                                            "afsk_live_reset", "afsk_live_destroy"}
    assert set(_native.LIVE_MIXED_SIGNATURES) == {"afsk_live_create_mixed", "afsk_live_tx_create_mixed",
                                                  "afsk_live_tx_state_bytes_mixed"}
    assert set(_native.LIVE_STREAM_SIGNATURES) == {"afsk_live_stream_layout", "afsk_live_create_stream"}
    assert len(_native.SIGNATURES) == 24 and len(_native.SPLIT_SIGNATURES) == 5 and len(_native.LIVE_TX_SIGNATURES) == 7
    for other in (_native.SIGNATURES, _native.SPLIT_SIGNATURES, _native.LIVE_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                  _native.LIVE_MIXED_SIGNATURES, _native.LIVE_STREAM_SIGNATURES, _native.LIVE_CLASS_SIGNATURES):
        assert not set(THRESHOLD_ENTRIES) & set(other)


def test_library_exports_threshold_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in THRESHOLD_ENTRIES + ("afsk_live_squelch_classes",):
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2


@pytest.mark.parametrize("kind", [STORED, STREAM])
def test_argument_checks_before_any_device(kind):
    lib = _native.lib()
    fn = getattr(lib, kind[0])
    (b, bp), (s, sp), (e, ep) = arr([40, 160]), arr([18000, 9000]), arr([14000, 7000])
    h = C.c_void_p(1234)
    for args in ((None, sp, ep), (bp, None, ep), (bp, sp, None)):
        assert fn(2, *args, kind[1], 8192, C.byref(h)) == _native.E_INVALID_ARG
        assert not h
    for n in (0, -1):
        assert fn(n, bp, sp, ep, kind[1], 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert fn(2, bp, sp, ep, kind[1], 8192, None) == _native.E_INVALID_ARG
    for bad in (0, 6, 41, 2048, -40):
        assert create(kind, [40, bad], [18000, 9000], [14000, 7000]) == _native.E_INVALID_BAUD
    # the capacities are the scalar entries'
    caps = ((4095, 8192), (96000, 0)) if kind is STORED else ((-1, 8192), (65537, 8192), (256, 0))
    for cap, chunk in caps:
        assert create(kind, [40, 160], [18000, 9000], [14000, 7000], cap, chunk) == _native.E_INVALID_ARG
    # a valid request gets as far as the device
    assert create(kind, [40, 160], [18000, 9000], [14000, 7000]) in (_native.OK, _native.E_NO_DEVICE)
    assert create(kind, [40, 40], [18000, 18000], [14000, 14000]) in (_native.OK, _native.E_NO_DEVICE)


def test_stored_receiver_caps_distinct_amp_end_at_16():
    n = 40
    end16 = [14000 - (c % 16) for c in range(n)]
    end17 = [14000 - (c % 17) for c in range(n)]
    start = [18000 + c for c in range(n)]                   # amp_start: any number of distinct values
    for bf in ([40] * n, [(4, 20, 40, 160, 2000)[c % 5] for c in range(n)]):
        assert create(STORED, bf, start, end16) in (_native.OK, _native.E_NO_DEVICE)
        assert create(STORED, bf, start, end17) == _native.E_INVALID_ARG
        msg = _native.last_error()
        assert "afsk_live_create_stream_thresholds" in msg and "streaming" in msg
        assert create(STREAM, bf, start, end17) in (_native.OK, _native.E_NO_DEVICE)
    assert create(STREAM, [40] * 2048, [18000] * 2048, list(range(2048))) in (_native.OK, _native.E_NO_DEVICE)


def test_python_sequences_of_the_wrong_length():
    for bad in ([18000] * 3, [18000] * 5, [[18000, 1], [2, 3]], np.full(3, 18000)):
        with pytest.raises(ValueError):
            live.LiveReceiver(4, 40, amp_start_threshold=bad)
        with pytest.raises(ValueError):
            live.LiveReceiver(4, [40, 80, 160, 40], amp_end_threshold=bad)
        with pytest.raises(ValueError):
            live.LiveReceiver(4, 40, amp_end_threshold=bad, max_burst_len=None)


class Recorder:
    """Stands in for the library: records what the constructor hands to the create entries, then stops it."""

    class Stop(Exception):
        pass

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in THRESHOLD_ENTRIES:
            def entry(n, bf, start, end, cap, chunk, out):
                take = lambda p: np.ctypeslib.as_array(p, (n,)).copy()  # noqa: E731
                self.calls.append((name, n, take(bf), take(start), take(end), cap, chunk))
                raise Recorder.Stop()
            return entry
        if name.startswith("afsk_live_create"):
            raise AssertionError(f"the constructor called {name}")
        return getattr(self.real, name)


@pytest.fixture
def recorded(monkeypatch):
    rec = Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    monkeypatch.setattr(batch._NativePlan, "__init__", lambda self, device=None: setattr(self, "_h", C.c_void_p())
                        or setattr(self, "device", "cpu"))
    import contextlib
    torch = batch._torch()
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    return rec


def build(rec, make):
    with pytest.raises(Recorder.Stop):
        make()
    return rec.calls[-1]


def test_constructor_hands_over_per_channel_arrays(recorded):
    name, n, bf, start, end, cap, chunk = build(recorded, lambda: live.LiveReceiver(
        3, [40, 160, 80], amp_start_threshold=[18000, 9000.7, 5406], amp_end_threshold=(14000, 7000, 4226.2)))
    assert name == "afsk_live_create_thresholds" and n == 3 and cap == live.DEFAULT_MAX_BURST_LEN
    assert bf.tolist() == [40, 160, 80] and start.tolist() == [18000, 9000, 5406] and end.tolist() == [14000, 7000, 4227]
    name, n, bf, start, end, cap, chunk = build(recorded, lambda: live.LiveReceiver(
        2, 40, 18000, np.array([14000, 9000]), max_burst_len=None, max_payload_len=64))
    assert name == "afsk_live_create_stream_thresholds" and cap == 64
    assert bf.tolist() == [40, 40] and start.tolist() == [18000, 18000] and end.tolist() == [14000, 9000]
    # scalars still arrive, as arrays of one value (the C entry then builds the scalar receiver)
    name, n, bf, start, end, cap, chunk = build(recorded, lambda: live.LiveReceiver(2, 40))
    assert start.tolist() == [18000, 18000] and end.tolist() == [14000, 14000]


def test_from_receivers_shared_and_per_channel(recorded):
    rs = [afskmodem.Receiver(1200), afskmodem.Receiver(300, 9010, 7044), afskmodem.Receiver(2400, 18000, 9000)]
    with pytest.raises(ValueError, match="thresholds differ"):
        live.LiveReceiver.from_receivers(rs)
    with pytest.raises(ValueError, match="thresholds differ"):
        live.LiveReceiver.from_receivers(rs, thresholds="shared")
    with pytest.raises(ValueError):
        live.LiveReceiver.from_receivers(rs, thresholds="each")
    with pytest.raises(ValueError):
        live.LiveReceiver.from_receivers([], thresholds="per_channel")
    for kw, entry in (({}, "afsk_live_create_thresholds"),
                      ({"max_burst_len": None}, "afsk_live_create_stream_thresholds")):
        name, n, bf, start, end, cap, chunk = build(
            recorded, lambda: live.LiveReceiver.from_receivers(rs, thresholds="per_channel", max_chunk_len=4096, **kw))
        assert name == entry and n == 3 and chunk == 4096
        assert bf.tolist() == [40, 160, 20] and start.tolist() == [18000, 9010, 18000]
        assert end.tolist() == [14000, 7044, 9000]
    # Receiver.live stays the scalar pair for every channel
    name, n, bf, start, end, cap, chunk = build(recorded, lambda: afskmodem.Receiver(300, 9010, 7044).live(5))
    assert n == 5 and set(bf.tolist()) == {160} and set(start.tolist()) == {9010} and set(end.tolist()) == {7044}


def fields_of(**kw):
    """The host-side attributes of a LiveReceiver (set before anything native is called): without a device the
    constructor ends in the no-device error and nothing else; with one the receiver is built and closed again."""
    rx = object.__new__(live.LiveReceiver)
    try:
        live.LiveReceiver.__init__(rx, **kw)
    except _native.AfskNativeError as e:
        assert e.code == _native.E_NO_DEVICE
    else:
        rx.close()
    return rx


def test_threshold_attributes():
    rx = fields_of(n_channels=3, bit_frames=40, amp_start_threshold=[18000, 18000.9, 18000],
                   amp_end_threshold=[14000, 9000, 14000])
    assert rx.channel_amp_start.dtype == np.int32 and rx.channel_amp_start.tolist() == [18000] * 3
    assert rx.channel_amp_end.dtype == np.int32 and rx.channel_amp_end.tolist() == [14000, 9000, 14000]
    assert rx.amp_start_threshold == 18000 and rx.amp_end_threshold is None
    rx = fields_of(n_channels=2, bit_frames=[40, 160])
    assert rx.channel_amp_start.tolist() == [18000, 18000] and rx.channel_amp_end.tolist() == [14000, 14000]
    assert rx.amp_start_threshold == 18000 and rx.amp_end_threshold == 14000
    rx = fields_of(n_channels=2, bit_frames=40, amp_start_threshold=[1, 2], amp_end_threshold=7000.5,
                   max_burst_len=None)
    assert rx.amp_start_threshold is None and rx.amp_end_threshold == 7001 and rx.channel_amp_end.tolist() == [7001] * 2


def test_nan_and_inf_entries_behave_as_the_scalars_do():
    vals = [math.nan, math.inf, -math.inf, 17999.5, -3.5, 18000]
    rx = fields_of(n_channels=len(vals), bit_frames=40, amp_start_threshold=vals, amp_end_threshold=vals)
    assert rx.channel_amp_start.tolist() == [batch.threshold_gt(v) for v in vals]
    assert rx.channel_amp_end.tolist() == [batch.threshold_lt(v) for v in vals]
    for v in vals:                                   # a sequence of one value is the scalar
        one = fields_of(n_channels=2, bit_frames=40, amp_start_threshold=v, amp_end_threshold=v)
        seq = fields_of(n_channels=2, bit_frames=40, amp_start_threshold=[v, v], amp_end_threshold=[v, v])
        assert one.channel_amp_start.tolist() == seq.channel_amp_start.tolist() == [batch.threshold_gt(v)] * 2
        assert one.amp_end_threshold == seq.amp_end_threshold == batch.threshold_lt(v)


@pytest.mark.parametrize("seed", range(6))
def test_squelch_classes_partition_the_slots(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    slots = int(rng.integers(1, 5))
    k = int(rng.integers(1, 17))
    values = rng.choice(np.arange(-5, 40000), k, replace=False)
    end = values[rng.integers(0, k, n)].astype(np.int32)
    rates = (4, 20, 40, 160, 2000, 80)[: int(rng.integers(1, 7))]
    bf = np.asarray([rates[i] for i in rng.integers(0, len(rates), n)], np.int32)
    classes = live.squelch_classes(bf, end, slots)
    assert [c[0] for c in classes] == list(dict.fromkeys(end.tolist()))      # distinct values, by first appearance
    seen = np.concatenate([c[2] for c in classes])
    assert seen.size == n * slots and np.array_equal(np.sort(seen), np.arange(n * slots))   # disjoint, complete
    for amp_end, uniform_bf, lst in classes:
        chans = lst // slots
        assert np.all(end[chans] == amp_end)
        assert np.array_equal(np.sort(lst), np.sort((np.nonzero(end == amp_end)[0][:, None] * slots
                                                     + np.arange(slots)[None, :]).reshape(-1)))
        cr = set(bf[chans].tolist())
        assert uniform_bf == (cr.pop() if len(cr) == 1 else 0)
        if len(set(bf[chans].tolist())) >= 4:                # rate by rate inside windows of 4096 entries
            for w in range(0, lst.size, 4096):
                r = bf[chans[w: w + 4096]]
                assert np.all(np.diff(r) >= 0)
        else:
            assert np.all(np.diff(lst) > 0)


def test_squelch_classes_windows_and_cap():
    n, slots = 9000, 2
    end = np.where(np.arange(n) % 3 == 0, 9000, 14000).astype(np.int32)
    bf = np.asarray([(4, 20, 40, 160, 2000)[c % 5] for c in range(n)], np.int32)
    classes = live.squelch_classes(bf, end, slots)
    assert [(c[0], c[1], c[2].size) for c in classes] == [(9000, 0, 6000), (14000, 0, 12000)]
    for _, _, lst in classes:
        for w in range(0, lst.size, 4096):
            win = lst[w: w + 4096]
            assert np.all(np.diff(bf[win // slots]) >= 0)
            assert w == 0 or win.min() > lst[w - 4096: w].max()          # windows walk the slots front to back
    with pytest.raises(_native.AfskNativeError) as ei:
        live.squelch_classes([40] * 17, list(range(17)), 1)
    assert ei.value.code == _native.E_INVALID_ARG
    assert len(live.squelch_classes([40] * 16, list(range(16)), 1)) == 16
