"""Host side of the faded live medium (no GPU): the C-ABI declarations, their signature table and the library's exports;
``medium_fade_q15``, ``medium_fades``, ``fade_design``, ``from_matrix(fade=, fade_offset=)``; every refusal of
``afsk_live_mix_faded_check`` with its message; and the numpy model (tests/live_fade_model.py) against the filtered
model with a unity track, at the knots and just before them, and over cut ticks."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_fade_model as FD
from tests import live_fir_model as F
from tests import live_mix_model as M
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_mix_faded", "afsk_live_mix_faded_check")
U = M.UNITY
Q = 16384
BAD = _native.E_INVALID_ARG


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_FADE_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_FADE_SIGNATURES[name]
        params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        want = declared_args(hdr.replace("uint32_t noise", "int32_t noise"), name)
        assert res is C.c_int and len(args) == len(want) == params.count(",") + 1, name
        for a, w, p in zip(args, want, params.split(",")):
            if "uint32_t noise" in p:
                assert a is C.c_uint32, (name, p)
            else:
                assert a is w or (w is C.c_void_p and issubclass(a, C._Pointer)), (name, p)
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_mix_filtered_check(")
    # the faded mix: the filtered mix's list with the five fade arrays and their two counts in front of the stream
    f = list(_native.LIVE_FIR_SIGNATURES["afsk_live_mix_filtered"][1])
    assert _native.LIVE_FADE_SIGNATURES["afsk_live_mix_faded"][1] == \
        f[:-1] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32] + f[-1:]
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_FADE_SIGNATURES"]
    assert len(others) >= 21 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert (_native.LIVE_FADE_MAX_KNOTS, _native.LIVE_FADE_MIN_SHIFT, _native.LIVE_FADE_MAX_SHIFT) == (65536, 3, 15)


def test_library_exports_and_binds_both_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_FADE_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


# ------------------------------------------------------------------------------------------------ the Python layer

def test_int_knots_are_q15_and_float_knots_are_rounded_to_it():
    assert live.medium_fade_q15([32768], 8) == ([32768], 3) and live.medium_fade_q15([1.0], 32768) == ([32768], 15)
    assert live.medium_fade_q15([0.5, 0.25, np.float32(0.125), np.uint16(3)], 64) == ([16384, 8192, 4096, 3], 6)
    assert live.medium_fade_q15([0, 65535], 2048) == ([0, 65535], 11)
    assert live.medium_fade_q15([1.999969482421875, 0.0], 512 / 48000) == ([65535, 0], 9)     # the period in seconds
    assert len(live.medium_fade_q15([1] * 65536, 8)[0]) == 65536
    for bad in ([True], ["1"], [None], [[1]]):
        with pytest.raises(TypeError):
            live.medium_fade_q15(bad, 8)
    for bad, word in (([], "knots"), ([1] * 3, "knots"), ([1] * 65537, "knots"), ([65536], "knot must lie"),
                      ([-1], "knot must lie"), ([2.0], "knot must lie"), ([float("nan")], "finite")):
        with pytest.raises(ValueError, match=word):
            live.medium_fade_q15(bad, 8)


def test_a_period_is_samples_or_seconds_and_a_power_of_two():
    for n in (8, 16, 1024, 32768):
        assert live.medium_fade_period(n) == n and live.medium_fade_period(n / 48000) == n
    for bad in (0, 4, 7, 9, 12, 48000, 65536, -8, 1.0, 0.0):
        with pytest.raises(ValueError, match="power of two in 8 ... 32768"):
            live.medium_fade_period(bad)
    for bad in (True, "8", None):
        with pytest.raises(TypeError):
            live.medium_fade_period(bad)


def test_an_offset_is_samples_mod_2_32_or_seconds():
    assert live.medium_fade_offset(0) == 0 and live.medium_fade_offset(2 ** 32 + 5) == 5
    assert live.medium_fade_offset(-1) == 2 ** 32 - 1 and live.medium_fade_offset(0.5) == 24000
    assert live.medium_fade_offset(-0.001) == 2 ** 32 - 48
    with pytest.raises(TypeError):
        live.medium_fade_offset(True)


def test_the_fade_sibling_keeps_the_order_of_medium_csr():
    links = [(2, 5, 1.0, 9, 1, 0, 7), (0, 1, 0.5), (2, 3, U, 0.001, None, None), (0, 0, -1.0, 4), (2, 5, 0.25, 10, 0, 3),
             (0, 1, 1, 0, 7, -1, 2 ** 32 + 1), (0, 2, 1, 0, None, 2, -1)]
    rp, ls, lg = live.medium_csr(3, links)
    assert rp.tolist() == [0, 4, 4, 7] and ls.tolist() == [1, 0, 1, 2, 5, 3, 5]
    fade, off = live.medium_fades(3, links)
    assert fade.tolist() == [-1, -1, -1, 2, 0, -1, 3] and fade.dtype == np.int32
    assert off.tolist() == [0, 0, 1, 2 ** 32 - 1, 7, 0, 0] and off.dtype == np.uint32
    assert live.medium_filters(3, [x[:5] for x in links]).tolist() == [-1, -1, 7, -1, 1, -1, 0]
    assert all(a.size == 0 for a in live.medium_fades(2, []))
    assert live.medium_fades(1, [(0, 0, U, 0, None, -5)])[0].tolist() == [-5]       # (the range is the checker's business)
    for bad in ([(3, 0, U, 1, 0, 0)], [(0, 0)], [(0, 0, U, 1, 2, 3, 4, 5)]):
        with pytest.raises(ValueError):
            live.medium_fades(3, bad)
    for bad in (True, 1.0, "0"):
        with pytest.raises(TypeError):
            live.medium_fades(3, [(0, 0, U, 0, None, bad)])


def test_from_matrix_takes_one_track_or_a_matrix_and_spreads_the_offsets():
    gain = [[0, 1.0, 0], [0.5, 0, 0.25], [0, 1.0, 0]]
    P = 2
    plain = live.medium_matrix_links(gain, P)
    assert live.medium_matrix_links(gain, P, delay=5, filter=1) == \
        live.medium_matrix_links(gain, P, delay=5, filter=1, fade=None, fade_offset=None)
    n_src, n_out, links = live.medium_matrix_links(gain, P, fade=1)
    assert (n_src, n_out) == plain[:2] and links == [x + (0, None, 1, 0) for x in plain[2]]
    links = live.medium_matrix_links(gain, P, delay=480, filter=0, fade=2, fade_offset=0.25)[2]
    assert links == [x + (480, 0, 2, 12000) for x in plain[2]]
    links = live.medium_matrix_links(gain, P, fade=0, fade_offset="spread")[2]
    assert [x[6] for x in links] == [(k * 0x9E3779B1) % 2 ** 32 for k in range(len(links))]
    assert len({x[6] for x in links}) == len(links) and live.MEDIUM_FADE_SPREAD == FD.SPREAD
    # "spread" follows the CSR index: the arrays come out in the order the links went in
    fade, off = live.medium_fades(n_out, links)
    assert off.tolist() == [x[6] for x in links] and (fade == 0).all()
    fm = [[0, 1, 2, None], [3, 4, -1, 0], [6, 7, 8, 1]]                # three stations and one extra group
    om = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 0.001]]
    n_src, n_out, links = live.medium_matrix_links(gain, P, extra=1, delay=[[1, 2, 3, 4]] * 3, fade=fm, fade_offset=om)
    want = {(0, 1): (1, 2), (1, 0): (3, 5), (1, 2): (None, 7), (2, 1): (7, 10), (0, 3): (None, 4), (1, 3): (0, 8),
            (2, 3): (1, 48)}
    assert (n_src, n_out) == (8, 6) and len(links) == len(want) * P
    for o, s, g, d, f, fd, fo in links:
        assert o % P == s % P and f is None and (fd, fo) == want[(o // P, s // P)] and d == s // P + 1, (o, s, fd, fo)
    for bad in (dict(fade=[[1, 2, 3]] * 3), dict(fade=[1, 2, 3]), dict(fade=0, fade_offset=[[1, 2, 3, 4]] * 2),
                dict(fade=0, fade_offset="scatter"), dict(fade_offset=5)):
        with pytest.raises(ValueError):
            live.medium_matrix_links(gain, P, extra=1, **bad)
    with pytest.raises(TypeError):
        live.medium_matrix_links(gain, P, fade=0.5)


def test_a_medium_checks_its_fades_before_it_needs_a_device():
    tr = ([U, U // 2], 1024)
    with pytest.raises(ValueError, match="no fades"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, None, 0)])
    with pytest.raises(_native.AfskNativeError, match="link 0 names track 1 outside -1 ... 0"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, None, 1)], fades=[tr])
    with pytest.raises(_native.AfskNativeError, match="link 0 names track -2"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, None, -2)], fades=[tr])
    with pytest.raises(ValueError, match="no filters"):
        live.LiveMedium(4, 2, [(0, 1, U, 5, 0, 0)], fades=[tr])
    with pytest.raises(TypeError):
        live.LiveMedium(4, 2, [], fades=[([True], 8)])
    with pytest.raises(ValueError, match="knots"):
        live.LiveMedium(4, 2, [], fades=[([1, 2, 3], 8)])
    with pytest.raises(ValueError, match="power of two in 8"):
        live.LiveMedium(4, 2, [], fades=[([1, 2], 100)])
    with pytest.raises(ValueError, match="knot must lie"):
        live.LiveMedium(4, 2, [], fades=[([65536], 8)])
    if _native.device_count() <= 0:
        # everything was decided and checked; only the device is missing
        for links, kw in (([(0, 1, U, 5, None, 0)], dict(fades=[tr])), ([(0, 1, U)], dict(fades=[tr])),
                          ([(0, 1, U, 3, 0, 0, 77)], dict(fades=[tr, ([0], 8)], filters=[[1.0]]))):
            with pytest.raises(_native.AfskNativeError, match="no HIP device"):
                live.LiveMedium(4, 2, links, **kw)


# ---------------------------------------------------------------------------------------------------- fade_design

@pytest.mark.parametrize("spec", [(256, 1024, 2.0, None, 0), (64, 4096, 1.0, None, 5), (1024, 256, 10.0, 4.0, 1),
                                  (128, 32768, 0.5, 0.0, 2), (16, 8, 2000.0, None, 3)])
def test_fade_design_is_the_written_out_sum_of_sinusoids(spec):
    knots, period = live.fade_design(*spec)
    assert period == spec[1] and len(knots) == spec[0] and all(isinstance(v, int) for v in knots)
    assert knots == FD.design(*spec)
    assert live.medium_fade_q15(knots, period) == (knots, period.bit_length() - 1)
    power = np.mean((np.asarray(knots) / 32768) ** 2)
    assert abs(power - 1) < 0.01 or max(knots) == 65535                           # unit mean power, up to the clip
    assert len(set(knots)) > 1


def test_fade_design_has_no_seam_and_knows_its_seed():
    spec = (64, 4096, 1.0, None, 5)
    knots, _ = live.fade_design(*spec)
    L = spec[0]
    # the same sinusoids one and two track lengths on, and before the track: the track repeats
    for shift in (L, 2 * L, -L):
        assert FD.design(*spec, at=np.arange(L) + shift) == knots
    # the step over the seam is one of the track's steps, not a jump
    steps = np.abs(np.diff(np.asarray(knots + knots[:1])))
    assert steps[-1] <= steps[:-1].max()
    assert live.fade_design(*spec) == (knots, 4096) and live.fade_design(64, 4096, 1.0, None, 6)[0] != knots
    assert live.fade_design(64, 4096 / 48000, 1.0, None, 5) == (knots, 4096)       # the period in seconds


def test_fade_design_covers_the_edges_and_refuses_what_it_cannot_make():
    assert live.fade_design(1, 8, 0.0) == ([32768], 8)                             # one knot: a constant
    assert live.fade_design(8, 1024, 0.0)[0] == [32768] * 8                        # no Doppler: nothing moves
    assert live.fade_design(8, 1024, 5.0)[0] == [32768] * 8                        # below the track's first harmonic
    strong = np.asarray(live.fade_design(256, 1024, 2.0, 1000.0)[0])               # nearly all line of sight
    assert np.abs(strong - 32768).max() < 0.15 * 32768
    rayleigh = np.asarray(live.fade_design(256, 1024, 2.0)[0])
    assert rayleigh.min() < 0.35 * 32768 < 1.5 * 32768 < rayleigh.max()            # deep fades and peaks
    for bad in (dict(n_knots=0), dict(n_knots=3), dict(n_knots=131072), dict(period=100), dict(period=4),
                dict(doppler_hz=-1.0), dict(doppler_hz=float("nan")), dict(k_factor=-1.0),
                dict(n_knots=4, period=8, doppler_hz=24000.0)):
        with pytest.raises(ValueError):
            live.fade_design(**dict(dict(n_knots=64, period=1024, doppler_hz=1.0), **bad))


# --------------------------------------------------------------------------------------- afsk_live_mix_faded_check

def check(row_ptr, link_src, link_gain, link_delay, link_filter, link_fade, n_src, hist_len, filter_ptr, taps, fade_ptr,
          fade_shift, n_fades=None, n_knots=None):
    p = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)  # noqa: E731
    rp, ls, lg, ld, lf, lfd, fp, qp, qs = (p(v) for v in (row_ptr, link_src, link_gain, link_delay, link_filter,
                                                         link_fade, filter_ptr, fade_ptr, fade_shift))
    tp = None if taps is None else np.ascontiguousarray(taps, np.int16)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    return _native.lib().afsk_live_mix_faded_check(
        ptr(rp), ptr(ls), ptr(lg), ptr(ld), ptr(lf), ptr(lfd), rp.size - 1, n_src, 0 if ls is None else ls.size,
        hist_len, ptr(fp), None if tp is None or tp.size == 0 else tp.ctypes.data_as(C.POINTER(C.c_int16)),
        fp.size - 1 if fp is not None else 0, 0 if tp is None else tp.size, ptr(qp), ptr(qs),
        (qp.size - 1 if qp is not None else 0) if n_fades is None else n_fades,
        (int(qp[-1]) if qp is not None else 0) if n_knots is None else n_knots)


TWO = dict(row_ptr=[0, 1, 2], link_src=[0, 1], link_gain=[U, U], n_src=2, link_delay=[0, 0], link_filter=[-1, 0],
           hist_len=16, filter_ptr=[0, 3], taps=[Q, 0, -Q])


def refused(word, **kw):
    args = dict(TWO, link_fade=[-1, 1], fade_ptr=[0, 4, 5], fade_shift=[3, 15])
    args.update(kw)
    assert check(**args) == BAD, kw
    err = _native.last_error()
    assert word in err and "afsk_live_mix_" in err, (kw, err)
    return err


def test_check_accepts_what_the_rule_allows():
    ok = dict(TWO, link_fade=[-1, 1], fade_ptr=[0, 4, 5], fade_shift=[3, 15])
    assert check(**ok) == 0, _native.last_error()
    assert check(**dict(ok, link_fade=[0, 0])) == 0 and check(**dict(ok, link_fade=[-1, -1])) == 0
    assert check(**dict(ok, fade_ptr=[0, 65536], fade_shift=[9], link_fade=[0, -1])) == 0
    assert check(**dict(ok, fade_ptr=[0], fade_shift=None, link_fade=[-1, -1])) == 0          # no tracks
    # no filters: filter_ptr = {0} is legal
    assert check(**dict(ok, link_filter=[-1, -1], filter_ptr=[0], taps=None)) == 0, _native.last_error()
    assert check([0, 0], None, None, None, None, None, 0, 8, [0], None, [0], None) == 0       # no links at all


def test_check_refuses_a_track_index_outside_the_table_and_names_the_link():
    for f in (-2, 2, 2 ** 31 - 1, -2 ** 31):
        assert f"link 1 names track {f} outside -1 ... 1" in refused("link 1", link_fade=[-1, f])
    refused("link 0 names track 0 outside -1 ... -1", link_fade=[0, -1], fade_ptr=[0], fade_shift=None)


def test_check_refuses_a_fade_ptr_that_does_not_start_at_0_and_rise_to_the_knot_count():
    refused("fade_ptr[0] must be 0", fade_ptr=[1, 5, 6], n_knots=6)
    refused("fade_ptr must end at n_knots = 6", n_knots=6)
    refused("above n_knots = 4 at track 1", n_knots=4)
    refused("track 1 has -2 knots", fade_ptr=[0, 4, 2], n_knots=4)
    refused("track 0 has 0 knots", fade_ptr=[0, 0, 4])
    refused("null fade_ptr", fade_ptr=None, n_fades=2, n_knots=5)
    refused("null fade_shift", fade_shift=None)
    refused("null link_fade", link_fade=None)
    refused("negative", n_fades=-1)
    refused("negative", n_knots=-1)


def test_check_refuses_a_knot_count_that_is_no_power_of_two_and_names_the_track():
    for n in (3, 5, 6, 7, 12, 65535, 65537, 131072):
        assert f"track 1 has {n} knots, not a power of two in 1 ... 65536" in refused("track 1", fade_ptr=[0, 4, 4 + n])
    for n in (1, 2, 64, 65536):
        assert check(**dict(TWO, link_fade=[-1, 1], fade_ptr=[0, 4, 4 + n], fade_shift=[3, 15])) == 0


def test_check_refuses_a_shift_outside_3_to_15_and_names_the_track():
    for p in (2, 16, 0, -1, 2 ** 31 - 1):
        assert f"track 0 has a shift of {p}, outside 3 ... 15" in refused("track 0", fade_shift=[p, 3])
    refused("track 1 has a shift of 16", fade_shift=[3, 16])


def test_check_keeps_the_earlier_rules():
    refused("hist_len", hist_len=12)
    refused("row_ptr[0]", row_ptr=[1, 1, 2])
    refused("link 1 names source 2", link_src=[0, 2])
    refused("link 0 has a gain", link_gain=[65536, U])
    refused("link 1 names filter 1", link_filter=[-1, 1])
    refused("link 1 has a reach", link_delay=[16, 15])
    refused("filter 0 has a sum of |taps|", taps=[32767, -32768, 1])
    refused("null filter_ptr", filter_ptr=None)


# ------------------------------------------------------------------------------------------------------- the model

LINKS = [(0, 0, U, 0, 0, 0, 5), (0, 1, U // 2, 3, 1, 1), (1, 2, -U, 8, None, 2, 2 ** 32 - 3), (1, 2, U // 4, 1, 2),
         (2, 0, 65535, 5, 0, 1, 1000), (2, 1, U, 7), (2, 2, 1, 0, 1, None), (2, 0, -U // 2, 2, None, 0), (2, 1, U, 6, 2, 2, 77),
         (4, 2, U, 4, 1, 1, 12345)]
FILTERS = [[Q], [Q // 2, -Q // 4, 3, -7, 1000], live.fir_design(9, 0, 6000)]
FADES = [([65535, 0, U, 1], 8), ([U // 2], 4096), ([40000, 100, 65535, 0, 7, U, U, 20000], 16)]


def tables(links=LINKS, n_out=5, filters=FILTERS, fades=FADES):
    fp = np.concatenate([[0], np.cumsum([len(h) for h in filters])]).astype(np.int32)
    qp = np.concatenate([[0], np.cumsum([len(k) for k, _ in fades])]).astype(np.int32)
    fade, off = live.medium_fades(n_out, links)
    return dict(zip(("row_ptr", "link_src", "link_gain_q15"), live.medium_csr(n_out, links)),
                link_delay=live.medium_delays(n_out, [x[:4] for x in links]),
                link_filter=live.medium_filters(n_out, [x[:5] for x in links]), filter_ptr=fp,
                filter_taps=np.asarray([t for h in filters for t in h], np.int16), link_fade=fade, link_fade_offset=off,
                fade_ptr=qp, fade_shift=np.asarray([live.medium_fade_q15(*f)[1] for f in fades], np.int32),
                fade_knots=np.asarray([v for k, _ in fades for v in k], np.uint16))


def mix(tl, src, t, n_out, T, **kw):
    names = ("link_filter", "filter_ptr", "filter_taps", "link_fade", "link_fade_offset", "fade_ptr", "fade_shift",
             "fade_knots")
    return tl.mix(src, t["row_ptr"], t["link_src"], t["link_gain_q15"], t["link_delay"], n_out, T,
                  **{n: t[n] for n in names if n in t}, **kw)


def test_the_model_with_a_unity_track_on_every_link_is_the_filtered_model():
    rng = np.random.default_rng(1)
    src = rng.integers(-32768, 32768, (3, 300), dtype=np.int16)
    src[:, :4] = [[-32768, 32767, -32768, 32767]] * 3
    t = tables([x[:5] + (None,) * (5 - len(x[:5])) + (0, 999 * i) for i, x in enumerate(LINKS)], fades=[([U] * 4, 8)])
    assert (t["link_fade"] == 0).all()
    plain = {k: v for k, v in t.items() if "fade" not in k}
    lens, scale = [300, 17, -4], [1 << 20, 0, 5 << 20, 1 << 22, 3]
    for hist_len in (16, 4096):
        a, b = FD.Timeline(3, hist_len, pos=40), F.Timeline(3, hist_len, pos=40)
        for T in (1, 9, 290):
            kw = dict(src_lens=lens, noise_scale_q24=scale, seed=5, noise_idx_base=9)
            got, want = mix(a, src, t, 5, T, **kw), mix(b, src, plain, 5, T, **kw)
            assert (got == want).all() and want.any(), (hist_len, T)


@pytest.mark.parametrize("p", [3, 4, 11, 15])
def test_the_envelope_is_the_knot_at_q_0_and_stays_short_of_the_next_at_the_last_q(p):
    knots = [65535, 0, U, 1, 40000, 40000, 7, 65535]
    L, per = len(knots), 1 << p
    at = np.arange(3 * L) * per                                                   # q = 0: the knot itself, cyclic
    assert FD.envelope(knots, p, at).tolist() == (knots * 3)
    assert FD.envelope(knots, p, at + 2 ** 32).tolist() == (knots * 3)            # u is taken mod 2^32
    last = FD.envelope(knots, p, at[:L] + per - 1)                                # q = 2^p - 1
    for n in range(L):
        a, b = knots[n], knots[(n + 1) % L]
        assert last[n] == a + (((b - a) * (per - 1)) >> p)
        assert min(a, b) <= last[n] <= max(a, b) and (last[n] != b or a >= b)     # floor: a rising pair stays short
    # a falling pair floors away from the start: 65535 -> 0 at q = 1 is 65535 + floor(-65535 / 2^p)
    assert FD.envelope(knots, p, [1])[0] == 65535 + ((-65535) >> p)
    # L * 2^p divides 2^32: the position's high bits do not matter
    u = np.asarray([5, per * L - 1, 2 ** 32 - 1, 2 ** 32 - per])
    assert (FD.envelope(knots, p, u) == FD.envelope(knots, p, u + 7 * 2 ** 32)).all()
    assert (FD.envelope(knots, p, u) == FD.envelope(knots, p, u % (per * L))).all()


def test_the_rule_floors_and_saturates_inside_the_gain():
    x = np.asarray([[3, -3, 1, -32768, 32767, -32768, -1, 0]], np.int16)
    fades = [([U], 8), ([65535], 8), ([1], 8), ([0], 8), ([U // 2], 8)]
    t = tables([(r, 0, U, 0, None, r) for r in range(5)] + [(5, 0, U // 2, 0, None, 1)], 6, [[Q]], fades)
    got = mix(FD.Timeline(1, 8), x, t, 6, 8)
    assert got[0].tolist() == x[0].tolist()                                       # unity: exact
    # 65535 * -32768 >> 15 = -65535: the inner clamp bites; 65535 * 32767 >> 15 = 65533 -> 32767
    assert got[1].tolist() == [5, -6, 1, -32768, 32767, -32768, -2, 0]
    assert got[2].tolist() == [0, -1, 0, -1, 0, -1, -1, 0]                         # e = 1: floor towards minus infinity
    assert not got[3].any()
    assert got[4].tolist() == [1, -2, 0, -16384, 16383, -16384, -1, 0]
    assert got[5].tolist() == [2, -3, 0, -16384, 16383, -16384, -1, 0]             # the gain behind the clamp


@pytest.mark.parametrize("hist_len,cuts,pos", [(16, [5, 8, 24, 1, 7, 55], 11), (16, [100], 11), (4096, [33, 67], 2 ** 32 - 40),
                                               (4096, [1] * 60, 2 ** 32 - 30), (16, [16] * 6 + [4], 2 ** 40 + 3)])
def test_tick_sequences_equal_one_tick_of_their_sum(hist_len, cuts, pos):
    rng = np.random.default_rng(2)
    total = sum(cuts)
    src = rng.integers(-32768, 32768, (3, total), dtype=np.int16)
    t = tables()
    kw = dict(noise_scale_q24=[1 << 20, 0, 5 << 20, 0, 1 << 22], seed=3, noise_idx_base=2)
    whole = mix(FD.Timeline(3, hist_len, pos=pos), src, t, 5, total, **kw)
    tl, parts, at = FD.Timeline(3, hist_len, pos=pos), [], 0
    for T in cuts:
        parts.append(mix(tl, src[:, at: at + T], t, 5, T, **kw))
        at += T
    assert (np.concatenate(parts, axis=1) == whole).all() and tl.pos == pos + total
    assert whole[:3].any() and whole[4].any() and not whole[3].any()
    # and the tracks matter: without them the rows differ
    plain = {k: v for k, v in t.items() if "fade" not in k}
    assert (mix(F.Timeline(3, hist_len, pos=pos), src, plain, 5, total, **kw) != whole).any()


def test_broken_tables_have_the_defined_result():
    x = np.full((1, 40), 20000, np.int16)
    base = tables([(0, 0, U, 0, None, 0)], 1, [[Q]], [([U // 2, U // 4, U, 0, 1, 2, 3, 4], 8)])

    def run(**kw):
        return mix(FD.Timeline(1, 8), x, dict(base, **{k: np.asarray(v) for k, v in kw.items()}), 1, 40)[0]
    good = run()
    assert good[0] == 10000 and good[8] == 5000 and good[4] == 7500
    assert not run(link_fade=[1]).any() and not run(link_fade=[-2]).any() and not run(link_fade=[2 ** 31 - 1]).any()
    assert (run(link_fade=[-1]) == 20000).all()
    assert (run(fade_shift=[2]) == good).all() and (run(fade_shift=[-5]) == good).all()       # clamped to 3
    assert (run(fade_shift=[16]) == run(fade_shift=[15])).all() and run(fade_shift=[16])[0] == 10000
    # 7 knots round down to 4, 3 to 2; none are silent; a fade_ptr beyond the knots is cut to them
    assert (run(fade_ptr=[0, 7]) == run(fade_ptr=[0, 4])).all() and run(fade_ptr=[0, 7])[32] == 10000
    assert (run(fade_ptr=[0, 3]) == run(fade_ptr=[0, 2])).all() and run(fade_ptr=[0, 3])[16] == 10000
    assert not run(fade_ptr=[0, 0]).any() and not run(fade_ptr=[5, 2]).any() and not run(fade_ptr=[9, 20]).any()
    assert (run(fade_ptr=[0, 100]) == good).all() and (run(fade_ptr=[-7, 8]) == good).all()
    assert run(fade_ptr=[6, 100])[0] == 3 * 20000 >> 15 and run(fade_ptr=[6, 100])[8] == 4 * 20000 >> 15   # knots 6, 7
