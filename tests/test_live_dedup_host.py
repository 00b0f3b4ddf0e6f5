"""The duplicate filter's rule on the CPU (no device): the key of tests/live_dedup_model.py against a second restatement and
against splitmix64's published outputs, what the key tells apart, the window's edges, the ring's replacement order, the
list-level rules (ineligible records, the unsorted tail, ``stored`` above ``max_events``), the state layout, and every
argument error of the Python layer that needs no device."""
import ctypes as C

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_dedup_model as D

OK, NO_DATA = _native.ST_OK, _native.ST_NO_DATA
W = 1000                                                 # a window in samples


def key_again(p: bytes) -> int:
    """The key once more, written as the header writes it: no shared helper with the model."""
    m = 2 ** 64

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) % m
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 % m
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB % m
        return z ^ (z >> 31)
    return mix(sum(mix(i * 256 + p[i]) for i in range(len(p))) % m ^ (len(p) * 2 ** 32) % m)


def test_mix64_is_the_splitmix64_output_function():
    # splitmix64 seeded with 0: its first two outputs (the generator adds the same increment before it mixes)
    assert D.mix64(0) == 0xE220A8397B1DCDAF
    assert D.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_the_key_matches_its_restatement_on_fixed_vectors():
    rng = np.random.default_rng(1)
    vectors = [b"\x00", b"\xff", b"A", b"Hello World!", bytes(range(256)), b"\x00" * 65, bytes(255), bytes(256)]
    vectors += [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (1, 6, 15, 16, 17, 63, 64, 65, 255, 256, 1000)]
    for p in vectors:
        assert D.key(p) == key_again(p), len(p)
        assert 0 <= D.key(p) < 2 ** 64
    assert D.key(b"\x00") == D.mix64(D.mix64(0) ^ (1 << 32))                     # one byte, by hand
    assert D.key(b"") == D.mix64(0)
    for length in (1, 6, 65):                                                    # the vectorised form the GPU tests preload with
        rows = rng.integers(0, 256, (50, length), dtype=np.uint8)
        assert D.keys_np(rows).tolist() == [D.key(bytes(r)) for r in rows]


def test_the_key_tells_near_payloads_apart():
    base = bytes(range(10, 34))
    seen = {D.key(base)}
    for i in range(len(base)):
        for bit in range(8):
            flipped = bytearray(base)
            flipped[i] ^= 1 << bit
            seen.add(D.key(bytes(flipped)))
    assert len(seen) == 1 + 8 * len(base)
    # permutations of the bytes (the sum runs over (index, byte) pairs, not over bytes)
    rng = np.random.default_rng(2)
    perms = {bytes(np.frombuffer(base, np.uint8)[rng.permutation(len(base))]) for _ in range(200)} | {base, base[::-1]}
    assert len({D.key(p) for p in perms}) == len(perms)
    assert D.key(b"ab") != D.key(b"ba")
    # trailing zero bytes: the length is part of the key
    zeros = [b"abc" + b"\x00" * k for k in range(6)] + [b"\x00" * k for k in range(1, 6)]
    assert len({D.key(p) for p in zeros}) == len(zeros)


def test_100000_random_six_byte_payloads_do_not_collide():
    rng = np.random.default_rng(3)
    pays = {bytes(r) for r in rng.integers(0, 256, (100000, 6), dtype=np.uint8)}
    assert len({D.key(p) for p in pays}) == len(pays) and len(pays) > 99990


def rows_of(items, pay_at=None):
    """Event rows (channel, burst_start, burst_len, flags, status, nbytes, payload_offset) and the payload part of
    ``items`` -- (channel, payload, end time) each, the payloads back to back."""
    rows, blob = [], b""
    for ch, p, t in items:
        rows.append((ch, t - 2048, 2048, 0, OK, len(p), len(blob)))
        blob += p
    return rows, blob


def run(model, items, window=W, max_events=None, stride=64, **kw):
    rows, blob = rows_of(items)
    me = len(rows) if max_events is None else max_events
    buf = D.events_buffer(rows, me, max(len(blob), 1), blob, **kw)
    return model.filter(buf, me, max(len(blob), 1), stride, window).tolist()


def test_the_window_edges():
    for age, want in ((W - 1, D.DUP), (W, D.NEW), (0, D.DUP), (-1, D.NEW), (-W, D.NEW)):
        m = D.DedupModel(2, 4)
        assert run(m, [(1, b"abcdef", 5000)]) == [D.NEW]
        assert run(m, [(1, b"abcdef", 5000 + age)]) == [want], age
    # a duplicate does not refresh: the second copy at age W - 1 leaves the entry's time, the third at W is new
    m = D.DedupModel(1, 4)
    assert run(m, [(0, b"x", 100)]) == [D.NEW] and run(m, [(0, b"x", 100 + W - 1)]) == [D.DUP]
    assert int(m.entries[0, 0]["time"]) == 100 and m.head[0] == 1
    assert run(m, [(0, b"x", 100 + W)]) == [D.NEW] and m.head[0] == 2
    # another channel's entry does not count
    assert run(m.copy(), [(0, b"x", 100 + W + 1)]) == [D.DUP]
    m2 = D.DedupModel(2, 4)
    assert run(m2, [(0, b"x", 100)]) == [D.NEW] and run(m2, [(1, b"x", 101)]) == [D.NEW]


def test_window_zero_remembers_everything_and_drops_nothing():
    m = D.DedupModel(1, 3)
    assert run(m, [(0, b"same", 10), (0, b"same", 10), (0, b"same", 11)], window=0) == [D.NEW] * 3
    assert [int(t) for t in m.entries[0]["time"]] == [10, 10, 11] and m.head[0] == 0
    assert len({int(k) for k in m.entries[0]["key"]}) == 1


@pytest.mark.parametrize("depth", [1, 2, 8, 64])
def test_depth_plus_one_distinct_payloads_push_the_first_one_out(depth):
    m = D.DedupModel(1, depth)
    pays = [bytes([65 + i % 26, i // 26 + 48]) for i in range(depth + 1)]
    assert run(m, [(0, p, 100 + i) for i, p in enumerate(pays)]) == [D.NEW] * (depth + 1)
    assert run(m.copy(), [(0, pays[0], 200)]) == [D.NEW]                        # replaced although it had not expired
    if depth > 1:
        assert run(m.copy(), [(0, pays[1], 200)]) == [D.DUP]
    assert run(m.copy(), [(0, pays[depth], 200)]) == [D.DUP]
    assert m.head[0] == 1 % depth


def test_two_equal_bursts_in_one_list_are_new_then_duplicate():
    m = D.DedupModel(3, 4)
    got = run(m, [(0, b"pq", 50), (0, b"pq", 60), (1, b"pq", 60), (1, b"rs", 61), (1, b"pq", 62)])
    assert got == [D.NEW, D.DUP, D.NEW, D.NEW, D.DUP]
    assert m.head.tolist() == [1, 2, 0]


def test_every_ineligible_kind_passes_and_leaves_the_table_unchanged():
    m = D.DedupModel(2, 2)
    assert run(m, [(0, b"seen", 10)]) == [D.NEW]
    before = (m.entries.copy(), m.head.copy())
    pay = b"seen" + bytes(60)
    rows = [(-1, 0, 20, 0, OK, 4, 0),                    # channel below the filter's
            (0, 0, 20, 0, NO_DATA, 4, 0),                # did not decode
            (0, 0, 20, 0, OK, 0, 0),                     # no byte
            (0, 0, 20, 0, OK, 9, 0),                     # a truncated streaming row: nbytes above out_stride
            (0, 0, 20, 0, OK, 4, -1),                    # the pack left the payload out
            (0, 0, 20, 0, OK, 4, 61),                    # ends past max_bytes
            (0, 0, 20, D.OVERFLOW, OK, 4, 0),
            (0, 0, 20, D.OPEN_END, OK, 4, 0),            # (the default skip_flags)
            (2, 0, 20, 0, OK, 4, 0)]                     # channel past the filter's
    buf = D.events_buffer(rows, len(rows), 64, pay)
    assert m.filter(buf, len(rows), 64, 8, W).tolist() == [D.PASS] * len(rows)
    assert (m.entries == before[0]).all() and (m.head == before[1]).all()
    # skip_flags = 0 makes the open-ended record eligible; OVERFLOW never is
    assert m.filter(buf, len(rows), 64, 8, W, skip_flags=0).tolist() == [D.PASS] * 7 + [D.DUP, D.PASS]
    assert m.filter(buf, len(rows), 64, 8, W, skip_flags=D.OVERFLOW).tolist() == [D.PASS] * 7 + [D.DUP, D.PASS]


def test_the_unsorted_tail_passes():
    m = D.DedupModel(4, 2)
    items = [(0, b"a", 1), (2, b"b", 2), (1, b"c", 3), (3, b"a", 4)]
    assert run(m, items) == [D.NEW, D.NEW, D.PASS, D.PASS]
    assert m.head.tolist() == [1, 0, 1, 0]


def test_stored_above_max_events_is_clamped_and_negative_is_none():
    items = [(0, b"a", 1), (1, b"b", 2), (2, b"c", 3)]
    m = D.DedupModel(4, 2)
    assert run(m, items, max_events=2, stored=77) == [D.NEW, D.NEW]
    assert run(D.DedupModel(4, 2), items, max_events=5, stored=2) == [D.NEW, D.NEW, D.NONE, D.NONE, D.NONE]
    assert run(D.DedupModel(4, 2), items, max_events=3, stored=-4) == [D.NONE] * 3


def test_note_follows_the_same_rule():
    m = D.DedupModel(3, 2)
    assert m.note([0, 0, 1], [b"hi", b"hi", b"hi"], [10, 11, 12], W).tolist() == [D.NEW, D.DUP, D.NEW]
    assert m.note([1, 0, 2], [b"x", b"y", b"z"], [1, 2, 3], W).tolist() == [D.NEW, D.PASS, D.PASS]          # descends at 1
    assert m.note([-1, 3, 2, 2], [b"x", b"x", b"", b"toolong"], [1] * 4, W, payload_stride=4).tolist() == [D.PASS] * 4
    assert m.note_any_order([2, 0, 9], [b"q", b"hi", b"q"], [20, 20, 20], W).tolist() == [D.NEW, D.DUP, D.PASS]
    m.reset([True, False, False])
    assert int(m.entries[0, 0]["time"]) == D.EMPTY and m.head.tolist() == [0, 0, 1]
    assert int(m.entries[1, 0]["time"]) == 12


def test_a_time_sum_wraps_like_int64():
    assert D.wrap64(2 ** 63 - 1 + 5) == -(2 ** 63) + 4 and D.wrap64(-5) == -5


# ------------------------------------------------------------------------------------------------ layout, arguments

def test_layout_values():
    assert live.dedup_layout(1, 1) == 256 + 256 + 256
    assert live.dedup_layout(16, 1) == 256 + 256 + 256
    assert live.dedup_layout(17, 1) == 512 + 256 + 256
    assert live.dedup_layout(65, 64) == 16 * 65 * 64 + 512 + 256
    assert live.dedup_layout(65536, 8) == 8 * 2 ** 20 + 4 * 65536 + 256           # 8 MiB of entries
    assert live.dedup_layout(2 ** 31 - 1, 64) == 16 * (2 ** 31 - 1) * 64 + 4 * 2 ** 31 + 256
    for n, depth in ((0, 8), (-1, 8), (4, 0), (4, 65), (4, -1)):
        with pytest.raises(_native.AfskNativeError) as ei:
            live.dedup_layout(n, depth)
        assert ei.value.code == _native.E_INVALID_ARG
    assert live.DEDUP_STATE_DTYPE.itemsize == 16 and live.DEDUP_EMPTY == D.EMPTY
    assert (_native.LIVE_DEDUP_NONE, _native.LIVE_DEDUP_DUP, _native.LIVE_DEDUP_NEW, _native.LIVE_DEDUP_PASS,
            _native.LIVE_TX_DUPLICATE) == (D.NONE, D.DUP, D.NEW, D.PASS, D.DUPLICATE)


def test_the_header_and_the_binding_agree():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "afsk_amd.h")).read()
    for name, value in (("AFSK_LIVE_DEDUP_NONE (-1)", D.NONE), ("AFSK_LIVE_DEDUP_DUP 0", D.DUP),
                        ("AFSK_LIVE_DEDUP_NEW 1", D.NEW), ("AFSK_LIVE_DEDUP_PASS 2", D.PASS),
                        ("AFSK_LIVE_TX_DUPLICATE 7", D.DUPLICATE)):
        assert "#define " + name in text, name
    for fn in _native.LIVE_DEDUP_SIGNATURES:
        assert "extern int " + fn + "(" in text, fn
        getattr(_native.lib(), fn)
    assert "remembered when it is HEARD" in text


def test_windows_are_seconds_or_samples():
    assert live.dedup_window(30.0) == 1440000 and live.dedup_window(30) == 30 and live.dedup_window(0) == 0
    assert live.dedup_window(0.5) == 24000 and live.dedup_window(np.int64(7)) == 7 and live.dedup_window(np.float32(1)) == 48000
    for bad in (True, "30", None, [1]):
        with pytest.raises(TypeError):
            live.dedup_window(bad)
    for bad in (-1, -0.5, float("inf"), float("nan"), 2 ** 63):
        with pytest.raises(ValueError):
            live.dedup_window(bad)


def test_constructor_errors_come_before_the_device_check():
    for kw in (dict(n_channels=0), dict(n_channels=4, depth=0), dict(n_channels=4, depth=65)):
        with pytest.raises(_native.AfskNativeError) as ei:
            live.LiveDedup(**kw)
        assert ei.value.code == _native.E_INVALID_ARG
    with pytest.raises(ValueError):
        live.LiveDedup(4, window=-1)
    with pytest.raises(TypeError):
        live.LiveDedup(4, window=True)


def test_call_errors_that_need_no_device():
    dd = live.LiveDedup.__new__(live.LiveDedup)                                  # (no device: never created)
    dd.n_channels, dd.depth, dd.window, dd.device = 4, 8, 100, "cpu"
    for skip in (4, 7, -1):
        with pytest.raises(ValueError):
            dd.filter(None, skip_flags=skip)
    with pytest.raises(ValueError):
        dd.filter(None, window=-5)
    with pytest.raises(TypeError):
        dd.filter(None, window="1")
    with pytest.raises(ValueError):
        dd.note([0, 1], [b"a"], 0)                                               # two channels, one payload
    with pytest.raises(ValueError):
        dd.note(0, [b"a", b"b"], [1, 2, 3])                                      # three times, two payloads
    with pytest.raises(ValueError):
        dd.note(0, [b"a"], 0, lengths=[1])                                       # lengths= belongs to a payload tensor
    with pytest.raises(ValueError):
        dd.note(0, [b"a"], 0, window=-1)
    # the C entries refuse a NULL filter before anything else
    lib = _native.lib()
    v = np.zeros(4, np.int32)
    assert lib.afsk_live_dedup_filter(None, v.ctypes.data, 4, 4, 4, 0, 0, v.ctypes.data, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_dedup_reset(None, None, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_dedup_destroy(None) == 0
    out = C.c_void_p(5)
    assert lib.afsk_live_dedup_create(4, 0, C.byref(out)) == _native.E_INVALID_ARG and not out
