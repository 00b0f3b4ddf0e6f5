"""Host side of the delayed live medium (no GPU): the C-ABI declarations, their signature table and the library's
exports; the numpy model over an explicit timeline (tests/live_delay_model.py) against tests/live_mix_model.py at delay
0, against itself over cut ticks, and against hand-worked delays; ``afsk_live_mix_delayed_check`` on a table of accept
and refuse cases; the delay sibling of ``medium_csr``, ``from_matrix(delay=)`` and seconds given as floats; and what
``live.LiveMedium`` decides before it needs a device."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_delay_model as D
from tests import live_mix_model as M
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_mix_delayed", "afsk_live_mix_delayed_check")
U = M.UNITY


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_DELAY_SIGNATURES) == set(ENTRIES)
    assert set(_native.LIVE_MIX_SIGNATURES) == {"afsk_live_mix", "afsk_live_mix_check"}
    for name in ENTRIES:
        res, args = _native.LIVE_DELAY_SIGNATURES[name]
        params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        want = declared_args(hdr.replace("uint32_t noise", "int32_t noise"), name)
        assert res is C.c_int and len(args) == len(want) == params.count(",") + 1, name
        for a, w, p in zip(args, want, params.split(",")):
            if "uint32_t" in p:
                assert a is C.c_uint32, (name, p)
            else:
                assert a is w or (w is C.c_void_p and issubclass(a, C._Pointer)), (name, p)
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_mix_check(")
    # the delayed mix: afsk_live_mix's list with the delays behind the gains, the history and its length behind pos
    mix = list(_native.LIVE_MIX_SIGNATURES["afsk_live_mix"][1])
    assert _native.LIVE_DELAY_SIGNATURES["afsk_live_mix_delayed"][1] == \
        mix[:7] + [C.c_void_p] + mix[7:16] + [C.c_void_p, C.c_int32] + mix[16:]
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_DELAY_SIGNATURES"]
    assert len(others) >= 19 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_library_exports_and_binds_both_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_DELAY_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


# ------------------------------------------------------------------------------------------------------- the model

LINKS = [(0, 0, U, 0), (0, 1, U // 2, 3), (1, 2, -U, 8), (1, 2, U // 4, 1), (2, 0, 65535, 5), (2, 1, U, 7), (2, 2, 1, 0),
         (2, 0, -U // 2, 2), (2, 1, U, 6), (4, 2, U, 4)]           # degrees 2, 2, 5, 0, 1


def tables(links=LINKS, n_out=5):
    return (*live.medium_csr(n_out, links), live.medium_delays(n_out, links))


def test_the_model_with_every_delay_0_is_the_undelayed_model():
    rng = np.random.default_rng(1)
    src = rng.integers(-32768, 32768, (3, 300), dtype=np.int16)
    rp, ls, lg, _ = tables()
    lens = [300, 17, -4]
    scale = [1 << 20, 0, 5 << 20, 1 << 22, 3]
    for hist_len in (8, 4096):
        tl = D.Timeline(3, hist_len, pos=40)
        pos = 40
        for T in (1, 9, 290):
            got = tl.mix(src, rp, ls, lg, np.zeros_like(ls), 5, T, src_lens=lens, noise_scale_q24=scale, seed=5,
                         noise_idx_base=9)
            want = M.mix(src, rp, ls, lg, 5, T, src_lens=lens, noise_scale_q24=scale, seed=5, noise_idx_base=9, pos=pos)
            assert (got == want).all(), (hist_len, T)
            pos += T
        assert tl.pos == pos


@pytest.mark.parametrize("hist_len,cuts", [(8, [5, 8, 24, 1, 7, 55]), (8, [100]), (16, [16] * 6 + [4]),
                                           (4096, [33, 67]), (4096, [1] * 100)])
def test_tick_sequences_equal_one_tick_of_their_sum(hist_len, cuts):
    rng = np.random.default_rng(2)
    total = sum(cuts)
    src = rng.integers(-32768, 32768, (3, total), dtype=np.int16)
    rp, ls, lg, ld = tables()
    scale = [1 << 20, 0, 5 << 20, 1 << 22, 0]
    kw = dict(noise_scale_q24=scale, seed=3, noise_idx_base=2)
    whole = D.Timeline(3, hist_len, pos=11).mix(src, rp, ls, lg, ld, 5, total, **kw)
    tl, parts, at = D.Timeline(3, hist_len, pos=11), [], 0
    for T in cuts:
        parts.append(tl.mix(src[:, at: at + T], rp, ls, lg, ld, 5, T, **kw))
        at += T
    assert (np.concatenate(parts, axis=1) == whole).all() and tl.pos == 11 + total
    assert whole[:4].any() and not M.mix(src, rp, ls, lg, 5, total)[3].any()


def test_a_delay_is_a_shift_that_reaches_into_earlier_ticks_and_a_length_cuts_what_was_sent():
    a = np.arange(1, 13, dtype=np.int16) * 100                     # one source: 100 ... 1200, sent in ticks of 4
    links = [(0, 0, U, 0), (1, 0, U, 1), (2, 0, U, 5), (3, 0, U, 8), (4, 0, U, 9), (5, 0, U // 2, 0), (5, 0, U, 3)]
    rp, ls, lg, ld = tables(links, 6)
    tl = D.Timeline(1, 8)
    got = np.concatenate([tl.mix(a[None, t: t + 4], rp, ls, lg, ld, 6, 4) for t in (0, 4, 8)], axis=1)
    shifted = lambda d: np.concatenate([np.zeros(d, np.int16), a])[:12]  # noqa: E731
    assert (got[0] == a).all() and (got[1] == shifted(1)).all() and (got[2] == shifted(5)).all()
    assert (got[3] == shifted(8)).all()
    assert (got[4] == shifted(8)).all()                             # a delay of 9 is clamped to hist_len = 8
    assert (got[5] == (a >> 1) + shifted(3)).all()                  # an echo: the source twice
    # columns at or beyond a length were never sent: they come back as zeros, whatever the buffer held there
    tl = D.Timeline(1, 8)
    first = tl.mix(a[None, :4], rp, ls, lg, ld, 6, 4, src_lens=[2])
    second = tl.mix(a[None, 4:8], rp, ls, lg, ld, 6, 4, src_lens=[9])
    assert first[0].tolist() == [100, 200, 0, 0] and first[1].tolist() == [0, 100, 200, 0]
    assert second[1].tolist() == [0, 500, 600, 700] and second[2].tolist() == [0, 100, 200, 0]


# -------------------------------------------------------------------------------------- afsk_live_mix_delayed_check

def check(row_ptr, link_src, link_gain, link_delay, n_src, hist_len, n_links=None):
    p = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)  # noqa: E731
    rp, ls, lg, ld = p(row_ptr), p(link_src), p(link_gain), p(link_delay)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    n_links = (0 if ls is None else ls.size) if n_links is None else n_links
    return _native.lib().afsk_live_mix_delayed_check(ptr(rp), ptr(ls), ptr(lg), ptr(ld), rp.size - 1, n_src, n_links,
                                                     hist_len)


@pytest.mark.parametrize("hist_len", [8, 16, 4096, 1 << 20])
def test_check_accepts_a_delay_inside_0_to_hist_len_only(hist_len):
    for d in (-1, 0, 1, hist_len - 1, hist_len, hist_len + 1):
        rc = check([0, 1, 2], [0, 1], [U, U], [0, d], 2, hist_len)
        if 0 <= d <= hist_len:
            assert rc == 0, (d, _native.last_error())
        else:
            assert rc == _native.E_INVALID_ARG, d
            err = _native.last_error()
            assert "afsk_live_mix_delayed_check" in err and "link 1" in err and f"delay of {d}" in err, err


@pytest.mark.parametrize("hist_len", [0, -8, 4, 7, 9, 12, 4095, (1 << 20) + 1, 1 << 21])
def test_check_refuses_a_hist_len_that_is_no_power_of_two_in_8_to_2_20(hist_len):
    assert check([0, 1], [0], [U], [0], 1, hist_len) == _native.E_INVALID_ARG
    assert "afsk_live_mix_delayed_check" in _native.last_error() and "hist_len" in _native.last_error()


def test_check_keeps_the_undelayed_rules():
    bad = _native.E_INVALID_ARG
    assert check([0, 0, 0], [], [], [], 4, 8) == 0 and check([0, 0], None, None, None, 0, 8) == 0
    for args, word in ((([1, 2], [0, 0], [U, U], [0, 0], 1), "row_ptr[0]"),
                       (([0, 2, 1, 3], [0, 0, 0], [U, U, U], [0, 0, 0], 1), "falls at output row 1"),
                       (([0, 1, 4], [0, 0, 0], [U, U, U], [0, 0, 0], 1), "end at n_links"),
                       (([0, 2], [0, 2], [U, U], [1, 1], 2), "link 1 names source 2"),
                       (([0, 2], [0, 0], [U, 65536], [1, 1], 1), "link 1 has a gain")):
        assert check(*args, 16) == bad and word in _native.last_error(), (word, _native.last_error())
    assert check([0, 1], [0], [U], None, 1, 8, n_links=1) == bad and "link_delay" in _native.last_error()
    assert check([0, 0], [], [], [], 1, 8, n_links=-1) == bad


# ------------------------------------------------------------------------------------------------ the Python layer

def test_float_delays_are_seconds_and_int_delays_samples():
    assert live.medium_delay(480) == 480 and live.medium_delay(np.int64(7)) == 7 and live.medium_delay(0) == 0
    assert live.medium_delay(0.01) == 480 and live.medium_delay(0.1) == 4800 and live.medium_delay(1.0) == 48000
    assert live.medium_delay(10 / 48000) == 10 and live.medium_delay(np.float32(0.5)) == 24000
    assert live.medium_delay(0.00001) == 0 and live.medium_delay(0.000011) == 1 == round(0.000011 * 48000)
    assert live.medium_delay(-0.001) == -48                         # (the range is the checker's business)
    for bad in (True, "1", None, [1]):
        with pytest.raises(TypeError):
            live.medium_delay(bad)
    with pytest.raises(ValueError):
        live.medium_delay(float("nan"))
    assert [live.medium_hist_len(d) for d in (0, 1, 8, 9, 16, 17, 4096, 4097, 1 << 20)] == \
        [8, 8, 8, 16, 16, 32, 4096, 8192, 1 << 20]


def test_the_delay_sibling_keeps_the_order_of_medium_csr():
    links = [(2, 5, 1.0, 9), (0, 1, 0.5), (2, 3, U, 0.001), (0, 0, -1.0, 4), (2, 5, 0.25, 10), (0, 1, 1, 0)]
    rp, ls, lg = live.medium_csr(3, links)                          # three arrays, as before
    ld = live.medium_delays(3, links)
    assert rp.tolist() == [0, 3, 3, 6] and ls.tolist() == [1, 0, 1, 5, 3, 5]
    assert lg.tolist() == [U // 2, -U, 1, U, U, U // 4]
    assert ld.tolist() == [0, 4, 0, 9, 48, 10] and ld.dtype == np.int32
    assert live.medium_delays(2, []).size == 0
    assert live.medium_delays(1, [(0, 0, U, 2 ** 40)]).tolist() == [2 ** 31 - 1]
    for bad in ([(3, 0, U, 1)], [(0, 0)], [(0, 0, U, 1, 2)]):
        with pytest.raises(ValueError):
            live.medium_delays(3, bad)
    with pytest.raises(TypeError):
        live.medium_delays(3, [(0, 0, U, True)])


def test_from_matrix_takes_one_delay_or_a_matrix_shaped_like_the_gains_and_the_extras():
    gain = [[0, 1.0, 0], [0.5, 0, 0.25], [0, 1.0, 0]]
    P = 2
    plain = live.medium_matrix_links(gain, P)
    assert all(len(x) == 3 for x in plain[2])                       # no delay asked for: triples, as before
    n_src, n_out, links = live.medium_matrix_links(gain, P, delay=480)
    assert (n_src, n_out) == plain[:2] and links == [x + (480,) for x in plain[2]]
    assert live.medium_matrix_links(gain, P, delay=0.01)[2] == links
    delay = [[1, 2, 3, 40], [4, 5, 6, 0.001], [7, 8, 9, 0]]          # three stations and one extra group
    n_src, n_out, links = live.medium_matrix_links(gain, P, extra=1, delay=delay)
    assert (n_src, n_out) == (8, 6)
    want = {(0, 1): 2, (1, 0): 4, (1, 2): 6, (2, 1): 8, (0, 3): 40, (1, 3): 48, (2, 3): 0}
    assert len(links) == len(want) * P
    for o, s, g, d in links:
        assert o % P == s % P and d == want[(o // P, s // P)], (o, s, d)
    ints = np.asarray([[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    assert [x[3] for x in live.medium_matrix_links(gain, 1, delay=ints)[2]] == [2, 4, 6, 8]
    for bad in ([[1, 2, 3]] * 3, [1, 2, 3], [[1, 2, 3, 4]] * 2):
        with pytest.raises(ValueError):
            live.medium_matrix_links(gain, P, extra=1, delay=bad)


def test_a_medium_decides_whether_it_is_delayed_before_it_needs_a_device():
    with pytest.raises(ValueError, match="above max_delay"):
        live.LiveMedium(4, 2, [(0, 1, U, 100)], max_delay=99)
    with pytest.raises(ValueError, match="above max_delay"):
        live.LiveMedium(4, 2, [(0, 1, U, 0.01)], max_delay=0.005)
    with pytest.raises(ValueError, match="max_delay"):
        live.LiveMedium(4, 2, [], max_delay=(1 << 20) + 1)
    with pytest.raises(ValueError, match="max_delay"):
        live.LiveMedium(4, 2, [], max_delay=-1)
    with pytest.raises(_native.AfskNativeError, match="delay of -3"):
        live.LiveMedium(4, 2, [(0, 1, U, -3)])
    with pytest.raises(_native.AfskNativeError, match="names source 4"):
        live.LiveMedium(4, 2, [(0, 4, U, 5)])
    with pytest.raises(ValueError):
        live.LiveMedium(4, 2, [(0, 1, U, 5, 6)])
    if _native.device_count() <= 0:
        for links, kw in (([(0, 1, U, 5)], {}), ([(0, 1, U)], dict(max_delay=0.1))):
            with pytest.raises(_native.AfskNativeError, match="no HIP device"):
                live.LiveMedium(4, 2, links, **kw)
