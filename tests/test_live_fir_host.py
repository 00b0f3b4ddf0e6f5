"""Host side of the filtered live medium (no GPU): the C-ABI declarations, their signature table and the library's
exports; ``medium_filter_q14``, ``medium_filters``, ``fir_design``, ``from_matrix(filter=)`` and ``hist_len`` from the
reach; every refusal of ``afsk_live_mix_filtered_check`` with its message; and the numpy model
(tests/live_fir_model.py) against the delayed model with the identity filter, against itself with a shifted delta and a
longer delay, and over cut ticks."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_delay_model as D
from tests import live_fir_model as F
from tests import live_mix_model as M
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_mix_filtered", "afsk_live_mix_filtered_check")
U = M.UNITY
Q = 16384
BAD = _native.E_INVALID_ARG


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_FIR_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_FIR_SIGNATURES[name]
        params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        want = declared_args(hdr.replace("uint32_t noise", "int32_t noise"), name)
        assert res is C.c_int and len(args) == len(want) == params.count(",") + 1, name
        for a, w, p in zip(args, want, params.split(",")):
            if "uint32_t" in p:
                assert a is C.c_uint32, (name, p)
            else:
                assert a is w or (w is C.c_void_p and issubclass(a, C._Pointer)), (name, p)
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_mix_delayed_check(")
    # the filtered mix: the delayed mix's list with the filter per link behind the delays, the table behind hist_len
    d = list(_native.LIVE_DELAY_SIGNATURES["afsk_live_mix_delayed"][1])
    assert _native.LIVE_FIR_SIGNATURES["afsk_live_mix_filtered"][1] == \
        d[:8] + [C.c_void_p] + d[8:19] + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + d[19:]
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_FIR_SIGNATURES"]
    assert len(others) >= 20 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert (_native.LIVE_FIR_MAX_TAPS, _native.LIVE_FIR_MAX_L1, _native.LIVE_FIR_UNITY) == (256, 65535, 16384)


def test_library_exports_and_binds_both_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_FIR_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


# ------------------------------------------------------------------------------------------------ the Python layer

def test_int_taps_are_q14_and_float_taps_are_rounded_to_it():
    assert live.medium_filter_q14([16384]) == [16384] and live.medium_filter_q14([1.0]) == [16384]
    assert live.medium_filter_q14([0.5, -0.25, np.float32(0.125), np.int16(-3), 0]) == [8192, -4096, 2048, -3, 0]
    assert live.medium_filter_q14([1 / 16384 * 0.49, -1.99993896484375]) == [0, -32767]
    assert live.medium_filter_q14([32767, -32768]) == [32767, -32768]               # sum of magnitudes: 65535
    assert len(live.medium_filter_q14([1] * 256)) == 256
    for bad in ([True], ["1"], [None], [[1]]):
        with pytest.raises(TypeError):
            live.medium_filter_q14(bad)
    for bad, word in (([], "taps"), ([1] * 257, "taps"), ([32768], "tap must lie"), ([-32769], "tap must lie"),
                      ([2.0], "tap must lie"), ([32767, -32768, 1], "65536"), ([16384] * 4, "65536"),
                      ([float("nan")], "finite")):
        with pytest.raises(ValueError, match=word):
            live.medium_filter_q14(bad)


def test_the_filter_sibling_keeps_the_order_of_medium_csr():
    links = [(2, 5, 1.0, 9, 1), (0, 1, 0.5), (2, 3, U, 0.001, None), (0, 0, -1.0, 4), (2, 5, 0.25, 10, 0), (0, 1, 1, 0, 7)]
    rp, ls, lg = live.medium_csr(3, links)
    assert rp.tolist() == [0, 3, 3, 6] and ls.tolist() == [1, 0, 1, 5, 3, 5]
    lf = live.medium_filters(3, links)
    assert lf.tolist() == [-1, -1, 7, 1, -1, 0] and lf.dtype == np.int32
    assert live.medium_filters(2, []).size == 0
    assert live.medium_filters(1, [(0, 0, U, 0, -5)]).tolist() == [-5]              # (the range is the checker's business)
    for bad in ([(3, 0, U, 1, 0)], [(0, 0)], [(0, 0, U, 1, 2, 3)]):
        with pytest.raises(ValueError):
            live.medium_filters(3, bad)
    for bad in (True, 1.0, "0"):
        with pytest.raises(TypeError):
            live.medium_filters(3, [(0, 0, U, 0, bad)])


# the issue's table: (taps, low, high) -> the sum of the magnitudes of the Q14 taps
DESIGNS = {(63, 0, 3000): 23062, (255, 300, 3000): 34615, (127, 300, 3400): 29552, (31, 0, 6000): 22572}


@pytest.mark.parametrize("spec,l1", sorted(DESIGNS.items()))
def test_fir_design_is_the_hamming_windowed_sinc_in_q14(spec, l1):
    h = live.fir_design(*spec)
    assert len(h) == spec[0] and all(isinstance(t, int) for t in h)
    assert h == h[::-1]                                                           # linear phase: symmetric taps
    assert sum(abs(t) for t in h) == l1 <= 65535
    assert h == F.design(*spec)
    if spec[1] == 0:                 # a low-pass passes 0 Hz: Hamming's ripple (0.2 %) plus K roundings of 2^-15 at most
        assert abs(sum(h) / Q - 1) < 0.005 + spec[0] / 32768


def test_fir_design_covers_the_edges_and_refuses_what_it_cannot_make():
    assert live.fir_design(1) == [16384]                                          # all-pass
    assert live.fir_design(1, 0, 12000) == [8192]
    assert live.fir_design(256, 0, 3000) == F.design(256, 0, 3000) and len(live.fir_design(2, 0, 100)) == 2
    for K in (2, 3, 16, 64, 255, 256):
        h = live.fir_design(K, 300, 3000)
        assert h == h[::-1] and sum(abs(t) for t in h) <= 65535
    for bad in (dict(n_taps=0), dict(n_taps=257), dict(n_taps=8, low_hz=3000, high_hz=3000),
                dict(n_taps=8, low_hz=-1), dict(n_taps=8, high_hz=24001), dict(n_taps=8, low_hz=5000, high_hz=300)):
        with pytest.raises(ValueError):
            live.fir_design(**bad)


def test_from_matrix_takes_one_filter_or_a_matrix_shaped_like_the_delays():
    gain = [[0, 1.0, 0], [0.5, 0, 0.25], [0, 1.0, 0]]
    P = 2
    plain = live.medium_matrix_links(gain, P)
    assert live.medium_matrix_links(gain, P, delay=5) == live.medium_matrix_links(gain, P, delay=5, filter=None)
    n_src, n_out, links = live.medium_matrix_links(gain, P, filter=1)
    assert (n_src, n_out) == plain[:2] and links == [x + (0, 1) for x in plain[2]]
    links = live.medium_matrix_links(gain, P, delay=480, filter=0)[2]
    assert links == [x + (480, 0) for x in plain[2]]
    filt = [[0, 1, 2, None], [3, 4, -1, 0], [6, 7, 8, 1]]              # three stations and one extra group
    n_src, n_out, links = live.medium_matrix_links(gain, P, extra=1, delay=[[1, 2, 3, 4]] * 3, filter=filt)
    want = {(0, 1): 1, (1, 0): 3, (1, 2): None, (2, 1): 7, (0, 3): None, (1, 3): 0, (2, 3): 1}
    assert (n_src, n_out) == (8, 6) and len(links) == len(want) * P
    for o, s, g, d, f in links:
        assert o % P == s % P and f == want[(o // P, s // P)] and d == s // P + 1, (o, s, d, f)
    assert live.medium_filters(n_out, links).min() == -1
    for bad in ([[1, 2, 3]] * 3, [1, 2, 3], [[1, 2, 3, 4]] * 2):
        with pytest.raises(ValueError):
            live.medium_matrix_links(gain, P, extra=1, filter=bad)
    with pytest.raises(TypeError):
        live.medium_matrix_links(gain, P, filter=0.5)


def test_a_medium_sizes_its_history_by_the_reach_before_it_needs_a_device():
    lp = live.fir_design(63, 0, 3000)
    with pytest.raises(ValueError, match="no filters"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, 0)])
    with pytest.raises(ValueError, match=r"reach .* of 162 samples, above max_delay = 161"):
        live.LiveMedium(4, 2, [(0, 1, U, 100, 0)], filters=[lp], max_delay=161)
    with pytest.raises(ValueError, match="above max_delay"):
        live.LiveMedium(4, 2, [(0, 1, U, 100)], filters=[lp], max_delay=99)
    with pytest.raises(_native.AfskNativeError, match="link 0 names filter 1 outside -1 ... 0"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, 1)], filters=[lp])
    with pytest.raises(_native.AfskNativeError, match="link 0 names filter -2"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, -2)], filters=[lp])
    with pytest.raises(_native.AfskNativeError, match="delay of -3"):
        live.LiveMedium(4, 2, [(0, 1, U, -3, 0)], filters=[lp])
    with pytest.raises(TypeError):
        live.LiveMedium(4, 2, [], filters=[[True]])
    with pytest.raises(ValueError, match="65535"):
        live.LiveMedium(4, 2, [], filters=[[16384] * 4])
    with pytest.raises(ValueError, match="taps"):
        live.LiveMedium(4, 2, [], filters=[[]])
    if _native.device_count() <= 0:
        # everything was decided and checked; only the device is missing
        for links, kw in (([(0, 1, U, 5, 0)], dict(filters=[lp])), ([(0, 1, U)], dict(filters=[[1.0]])),
                          ([(0, 1, U, 100, 0)], dict(filters=[lp], max_delay=162))):
            with pytest.raises(_native.AfskNativeError, match="no HIP device"):
                live.LiveMedium(4, 2, links, **kw)


# ------------------------------------------------------------------------------------- afsk_live_mix_filtered_check

def check(row_ptr, link_src, link_gain, link_delay, link_filter, n_src, hist_len, filter_ptr, taps, n_filters=None,
          n_taps=None, n_links=None):
    p = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)  # noqa: E731
    rp, ls, lg, ld, lf, fp = (p(v) for v in (row_ptr, link_src, link_gain, link_delay, link_filter, filter_ptr))
    tp = None if taps is None else np.ascontiguousarray(taps, np.int16)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    n_links = (0 if ls is None else ls.size) if n_links is None else n_links
    return _native.lib().afsk_live_mix_filtered_check(
        ptr(rp), ptr(ls), ptr(lg), ptr(ld), ptr(lf), rp.size - 1, n_src, n_links, hist_len, ptr(fp),
        None if tp is None or tp.size == 0 else tp.ctypes.data_as(C.POINTER(C.c_int16)),
        (fp.size - 1 if fp is not None else 0) if n_filters is None else n_filters,
        (0 if tp is None else tp.size) if n_taps is None else n_taps)


TWO = dict(row_ptr=[0, 1, 2], link_src=[0, 1], link_gain=[U, U], n_src=2)       # two links, one per row


def refused(word, **kw):
    args = dict(TWO, link_delay=[0, 0], link_filter=[-1, 0], hist_len=16, filter_ptr=[0, 3], taps=[Q, 0, -Q])
    args.update(kw)
    assert check(**args) == BAD, kw
    err = _native.last_error()
    assert word in err and ("afsk_live_mix_filtered_check" in err or "afsk_live_mix_" in err), (kw, err)
    return err


def test_check_accepts_what_the_rule_allows():
    ok = dict(TWO, link_delay=[16, 14], link_filter=[-1, 0], hist_len=16, filter_ptr=[0, 3], taps=[Q, 0, -Q])
    assert check(**ok) == 0, _native.last_error()                                 # reach 14 + 3 - 1 = hist_len
    assert check(**dict(ok, filter_ptr=[0, 1, 3], link_filter=[1, 0], link_delay=[15, 16])) == 0
    assert check(**dict(ok, link_filter=[-1, -1])) == 0
    assert check(**dict(ok, filter_ptr=[0, 2], taps=[32767, -32768], link_delay=[0, 15])) == 0
    assert check(**dict(ok, hist_len=256, filter_ptr=[0, 256], taps=[255] * 256, link_delay=[256, 1])) == 0
    assert check([0, 0], None, None, None, None, 0, 8, [0], None) == 0            # no links, no filters
    assert check([0, 0], None, None, None, None, 0, 8, [0, 1], [Q]) == 0


def test_check_refuses_a_filter_index_outside_the_table_and_names_the_link():
    for f in (-2, 1, 2 ** 31 - 1, -2 ** 31):
        assert f"link 1 names filter {f} outside -1 ... 0" in refused("link 1", link_filter=[-1, f])
    refused("link 0 names filter 0 outside -1 ... -1", link_filter=[0, -1], filter_ptr=[0], taps=None)


def test_check_refuses_a_filter_ptr_that_does_not_start_at_0_and_rise_to_the_tap_count():
    refused("filter_ptr[0] must be 0", filter_ptr=[1, 3])
    refused("filter_ptr must end at n_taps = 3", filter_ptr=[0, 2])
    refused("above n_taps = 3 at filter 0", filter_ptr=[0, 4])
    refused("filter 1 has -1 taps", filter_ptr=[0, 2, 1, 3])
    refused("filter 0 has 0 taps", filter_ptr=[0, 0, 3])
    refused("filter 1 has 0 taps", filter_ptr=[0, 3, 3])
    refused("null filter_ptr", filter_ptr=None, n_filters=1)
    refused("null filter_taps", taps=None, n_taps=3)
    refused("null link_filter", link_filter=None)
    refused("negative", n_filters=-1)
    refused("negative", n_taps=-1)


def test_check_refuses_k_outside_1_to_256_and_names_the_filter():
    refused("filter 0 has 257 taps, outside 1 ... 256", hist_len=512, filter_ptr=[0, 257], taps=[1] * 257)
    refused("filter 1 has 300 taps", hist_len=512, filter_ptr=[0, 1, 301], taps=[1] * 301)
    assert check(**dict(TWO, link_delay=[0, 0], link_filter=[-1, 0], hist_len=512, filter_ptr=[0, 256],
                        taps=[1] * 256)) == 0


def test_check_refuses_a_sum_of_magnitudes_above_65535_and_names_the_filter():
    refused("filter 0 has a sum of |taps| of 65536, above 65535", filter_ptr=[0, 3], taps=[32767, -32768, 1])
    refused("filter 1 has a sum of |taps| of 65536", filter_ptr=[0, 1, 3], taps=[Q, -32768, -32768], link_filter=[-1, -1])
    assert check(**dict(TWO, link_delay=[0, 0], link_filter=[0, 0], hist_len=16, filter_ptr=[0, 3],
                        taps=[-32768, -32767, 0])) == 0


def test_check_refuses_a_reach_above_hist_len_and_names_the_link():
    err = refused("link 1 has a reach", link_delay=[16, 15])                      # 15 + 3 - 1 = 17 > 16
    assert "of 17, above hist_len = 16" in err
    refused("link 1 has a reach", hist_len=8, filter_ptr=[0, 10], taps=[1] * 10)  # no delay: 9 > 8
    refused("delay of 17", link_delay=[17, 0])                                    # an unfiltered link: the delayed rule
    refused("delay of -1", link_delay=[0, -1])


def test_check_keeps_the_earlier_rules():
    refused("hist_len", hist_len=12)
    refused("row_ptr[0]", row_ptr=[1, 1, 2])
    refused("link 1 names source 2", link_src=[0, 2])
    refused("link 0 has a gain", link_gain=[65536, U])
    refused("link_delay", link_delay=None)


# ------------------------------------------------------------------------------------------------------- the model

LINKS = [(0, 0, U, 0, 0), (0, 1, U // 2, 3, 1), (1, 2, -U, 8, None), (1, 2, U // 4, 1, 2), (2, 0, 65535, 5, 0),
         (2, 1, U, 7), (2, 2, 1, 0, 1), (2, 0, -U // 2, 2, 2), (2, 1, U, 6, 2), (4, 2, U, 4, 1)]
FILTERS = [[Q], [Q // 2, -Q // 4, 3, -7, 1000], live.fir_design(9, 0, 6000)]


def tables(links=LINKS, n_out=5, filters=FILTERS):
    fp = np.concatenate([[0], np.cumsum([len(h) for h in filters])]).astype(np.int32)
    return dict(zip(("row_ptr", "link_src", "link_gain_q15"), live.medium_csr(n_out, links)),
                link_delay=live.medium_delays(n_out, [x[:4] for x in links]),
                link_filter=live.medium_filters(n_out, links), filter_ptr=fp,
                filter_taps=np.asarray([t for h in filters for t in h], np.int16))


def test_the_model_with_the_identity_filter_on_every_link_is_the_delayed_model():
    rng = np.random.default_rng(1)
    src = rng.integers(-32768, 32768, (3, 300), dtype=np.int16)
    t = tables([x[:4] + (0,) for x in LINKS], filters=[[Q]])
    assert (t["link_filter"] == 0).all()
    lens, scale = [300, 17, -4], [1 << 20, 0, 5 << 20, 1 << 22, 3]
    for hist_len in (8, 4096):
        a, b = F.Timeline(3, hist_len, pos=40), D.Timeline(3, hist_len, pos=40)
        for T in (1, 9, 290):
            kw = dict(src_lens=lens, noise_scale_q24=scale, seed=5, noise_idx_base=9)
            got = a.mix(src, t["row_ptr"], t["link_src"], t["link_gain_q15"], t["link_delay"], 5, T, **kw,
                        link_filter=t["link_filter"], filter_ptr=t["filter_ptr"], filter_taps=t["filter_taps"])
            want = b.mix(src, t["row_ptr"], t["link_src"], t["link_gain_q15"], t["link_delay"], 5, T, **kw)
            assert (got == want).all() and want.any(), (hist_len, T)


def mix(tl, src, t, n_out, T, **kw):
    return tl.mix(src, t["row_ptr"], t["link_src"], t["link_gain_q15"], t["link_delay"], n_out, T,
                  link_filter=t["link_filter"], filter_ptr=t["filter_ptr"], filter_taps=t["filter_taps"], **kw)


@pytest.mark.parametrize("n,d", [(0, 0), (1, 0), (5, 3), (255, 1), (7, 249)])
def test_zero_taps_in_front_of_unity_are_more_delay(n, d):
    rng = np.random.default_rng(n)
    src = rng.integers(-32768, 32768, (1, 700), dtype=np.int16)
    filtered = tables([(0, 0, 12345, d, 0)], 1, [[0] * n + [Q]])
    longer = tables([(0, 0, 12345, d + n)], 1, [[Q]])
    a, b = F.Timeline(1, 256), F.Timeline(1, 256)
    for at, T in ((0, 300), (300, 1), (301, 399)):
        got, want = mix(a, src[:, at: at + T], filtered, 1, T), mix(b, src[:, at: at + T], longer, 1, T)
        assert (got == want).all()
    assert want.any()


@pytest.mark.parametrize("hist_len,cuts", [(16, [5, 8, 24, 1, 7, 55]), (16, [100]), (16, [16] * 6 + [4]),
                                           (4096, [33, 67]), (4096, [1] * 60)])
def test_tick_sequences_equal_one_tick_of_their_sum(hist_len, cuts):
    rng = np.random.default_rng(2)
    total = sum(cuts)
    src = rng.integers(-32768, 32768, (3, total), dtype=np.int16)
    t = tables()
    kw = dict(noise_scale_q24=[1 << 20, 0, 5 << 20, 0, 1 << 22], seed=3, noise_idx_base=2)
    whole = mix(F.Timeline(3, hist_len, pos=11), src, t, 5, total, **kw)
    tl, parts, at = F.Timeline(3, hist_len, pos=11), [], 0
    for T in cuts:
        parts.append(mix(tl, src[:, at: at + T], t, 5, T, **kw))
        at += T
    assert (np.concatenate(parts, axis=1) == whole).all() and tl.pos == 11 + total
    assert whole[:3].any() and whole[4].any() and not whole[3].any()


def test_the_rule_floors_saturates_and_applies_the_gain_behind_the_filter():
    x = np.asarray([[3, -3, 1, -32768, -32768, 32767]], np.int16)
    t = tables([(0, 0, U, 0, 0), (1, 0, U, 0, 1), (2, 0, U // 2, 0, 1), (3, 0, U, 0, 2)], 4,
               [[Q // 2], [-32768, -32767], [32767, 32767]])
    got = mix(F.Timeline(1, 8), x, t, 4, 6)
    assert got[0].tolist() == [1, -2, 0, -16384, -16384, 16383]                   # v >> 14 floors: -1.5 -> -2
    # -32768 * -32768 + -32767 * -32768 = 2147450880 -> >> 14 = 131070 -> 32767; the mirror saturates at -32768
    assert got[1].tolist()[4] == 32767 and got[2].tolist()[4] == 16383
    assert got[3].tolist()[4] == -32768 and got[3].tolist()[5] == -2              # -32767 >> 14: floor
