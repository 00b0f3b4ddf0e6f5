"""Host side of the live medium (no GPU): the C-ABI declarations, their signature table and the library's exports; the
numpy model (tests/live_mix_model.py) against the torch-style expression it replaces and against hand-worked products;
the model's two noise paths against each other; ``afsk_live_mix_check`` on a table of accept and refuse cases; the CSR
and ``from_matrix`` expansion of ``live.LiveMedium``; and its no-device error."""
import ctypes as C
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_mix_model as M
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_mix", "afsk_live_mix_check")
U = M.UNITY


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_MIX_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_MIX_SIGNATURES[name]
        params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        want = declared_args(hdr.replace("uint32_t noise", "int32_t noise"), name)
        assert res is C.c_int and len(args) == len(want) == params.count(",") + 1, name
        for a, w, p in zip(args, want, params.split(",")):
            if "uint32_t" in p:
                assert a is C.c_uint32, (name, p)
            else:
                assert a is w or (w is C.c_void_p and issubclass(a, C._Pointer)), (name, p)
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_push_auto_muted(")
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_MIX_SIGNATURES"]
    assert len(others) >= 18 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2


def test_library_exports_and_binds_both_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_MIX_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


# ------------------------------------------------------------------------------------------------------- the model

def unity_csr(n_out, degree):
    """Output row r hears source rows r * degree ... r * degree + degree - 1 at unity."""
    return np.arange(n_out + 1) * degree, np.arange(n_out * degree), np.full(n_out * degree, U)


def test_the_model_at_unity_is_the_torch_style_expression():
    rng = np.random.default_rng(1)
    src = rng.integers(-32768, 32768, (12, 257), dtype=np.int16)
    src[0:3, :40] = 32767                                       # saturates upwards ...
    src[3:6, :40] = -32768                                      # ... and downwards
    got = M.mix(src, *unity_csr(4, 3), 4, 257)
    for r in range(4):
        assert (got[r] == M.torch_style(src[3 * r: 3 * r + 3])).all(), r
    assert (got[0, :40] == 32767).all() and (got[1, :40] == -32768).all()


def one(x, g):
    return int(M.mix(np.asarray([[x]], np.int16), [0, 1], [0], [g], 1, 1)[0, 0])


def test_products_round_towards_minus_infinity_and_the_corners_fit():
    assert one(-1, 1) == -1 and one(1, 1) == 0 and one(-1, -1) == 0 and one(1, -1) == -1      # floor, not truncation
    assert one(-32768, U) == -32768 and one(32767, U) == 32767
    assert one(-3, U // 2) == -2 and one(3, U // 2) == 1
    assert one(-32768, -U) == 32767                             # +32768 clips
    assert one(32767, 65535) == 32767 and one(-32768, 65535) == -32768 and one(-32768, -65535) == 32767
    assert one(16384, 65535) == (16384 * 65535) >> 15 == 32767
    assert one(16383, 65535) == 32765
    assert one(100, 70000) == one(100, 65535) and one(100, -70000) == one(100, -65535)          # the gain is clamped
    assert one(12345, 0) == 0


def test_the_model_clamps_and_ignores_a_broken_table_as_the_header_says():
    src = np.asarray([[100, 200, 300], [7, 8, 9]], np.int16)
    # a source outside the matrix is silent; a falling row_ptr gives an empty row; row_ptr beyond n_links is cut
    got = M.mix(src, [0, 2, 1, 9], [0, 5, 1], [U, U, U], 3, 3)
    assert got.tolist() == [[100, 200, 300], [0, 0, 0], [7, 8, 9]]
    got = M.mix(src, [-4, 2], [-1, 1], [U, U], 1, 3)
    assert got.tolist() == [[7, 8, 9]]
    # lengths: clamped to 0 ... T, and nothing beyond them is heard
    got = M.mix(src, [0, 2], [0, 1], [U, U], 1, 3, src_lens=[-5, 2])
    assert got.tolist() == [[7, 8, 0]]
    got = M.mix(src, [0, 2], [0, 1], [U, U], 1, 3, src_lens=[1, 12])
    assert got.tolist() == [[107, 8, 9]]


def test_both_noise_paths_of_the_model_agree_and_continue_over_a_cut():
    rng = np.random.default_rng(5)
    row = rng.integers(-20000, 20000, 700, dtype=np.int16)
    for pos, scale in ((0, 1 << 20), (1, 300000), (4099, 5 << 20), (M.ORACLE_MAX_POS, 1 << 28), (33, -(1 << 20))):
        want = M.noise_row(row, 77, 3, scale, pos)               # the oracle on pos zeros + the row
        assert (M.noise_direct(row, 77, 3, scale, pos) == want).all(), (pos, scale)
        assert (want != row).any()
    assert (M.noise_row(row, 77, 3, 1 << 28, 0) == 32767).any()  # noise that clips on its own
    whole = M.noise_row(row, 9, 1, 1 << 21, 100)
    halves = np.concatenate([M.noise_row(row[:300], 9, 1, 1 << 21, 100), M.noise_row(row[300:], 9, 1, 1 << 21, 400)])
    assert (whole == halves).all()
    assert (M.noise_row(row, 9, 1, 0, 5) == row).all()
    # the sample index wraps at 2^32: the samples behind the wrap are those of position 0
    at_wrap = M.noise_direct(row, 9, 1, 1 << 21, 2 ** 32 - 200)
    assert (at_wrap[200:] == M.noise_row(row[200:], 9, 1, 1 << 21, 0)).all()
    assert (at_wrap == M.noise_direct(row, 9, 1, 1 << 21, 2 ** 33 - 200)).all()
    out = M.mix(row[None, :], [0, 1, 2], [0, 0], [U, U // 2], 2, 700, noise_scale_q24=[1 << 20, 0], seed=4,
                noise_idx_base=10, pos=64)
    assert (out[0] == M.noise_row(row, 4, 10, 1 << 20, 64)).all() and (out[1] == row >> 1).all()


# --------------------------------------------------------------------------------------------- afsk_live_mix_check

def check(row_ptr, link_src, link_gain, n_src, n_out=None, n_links=None):
    p = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)  # noqa: E731
    rp, ls, lg = p(row_ptr), p(link_src), p(link_gain)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    n_out = rp.size - 1 if n_out is None else n_out
    n_links = (0 if ls is None else ls.size) if n_links is None else n_links
    return _native.lib().afsk_live_mix_check(ptr(rp), ptr(ls), ptr(lg), n_out, n_src, n_links)


ACCEPT = {
    "three rows": ([0, 2, 2, 5], [0, 1, 2, 0, 0], [U, -U, 1, 0, 65535], 3),
    "a duplicate link": ([0, 2], [1, 1], [U, U], 2),
    "no links": ([0, 0, 0], [], [], 4),
    "no links, no sources": ([0, 0], None, None, 0),
    "no rows": ([0], [], [], 3),
    "the extreme gains": ([0, 2], [0, 0], [-65535, 65535], 1),
    "32768 links in one row": ([0, 32768], [0] * 32768, [1] * 32768, 1),
}
REFUSE = {
    "row_ptr does not start at 0": (([1, 2], [0, 0], [U, U], 1), "row_ptr[0]"),
    "row_ptr falls": (([0, 2, 1, 3], [0, 0, 0], [U, U, U], 1), "falls at output row 1"),
    "row_ptr ends short": (([0, 1, 2], [0, 0, 0], [U, U, U], 1), "end at n_links"),
    "row_ptr ends beyond": (([0, 1, 4], [0, 0, 0], [U, U, U], 1), "end at n_links"),
    "32769 links in one row": (([0, 32769], [0] * 32769, [1] * 32769, 1), "more than 32768"),
    "a source at n_src": (([0, 2], [0, 2], [U, U], 2), "link 1 names source 2"),
    "a negative source": (([0, 2], [-1, 0], [U, U], 2), "link 0 names source -1"),
    "a link with no sources at all": (([0, 1], [0], [U], 0), "names source 0"),
    "a gain of 65536": (([0, 2], [0, 0], [U, 65536], 1), "link 1 has a gain"),
    "a gain of -65536": (([0, 1], [0], [-65536], 1), "link 0 has a gain"),
}


@pytest.mark.parametrize("case", list(ACCEPT))
def test_check_accepts(case):
    assert check(*ACCEPT[case]) == 0, _native.last_error()


@pytest.mark.parametrize("case", list(REFUSE))
def test_check_refuses_and_says_why(case):
    args, word = REFUSE[case]
    assert check(*args) == _native.E_INVALID_ARG
    assert "afsk_live_mix_check" in _native.last_error() and word in _native.last_error(), _native.last_error()


def test_check_refuses_null_arrays_and_negative_counts():
    bad = _native.E_INVALID_ARG
    assert check(None, [], [], 1, n_out=0) == bad and "row_ptr" in _native.last_error()
    assert check([0, 1], None, [U], 1, n_links=1) == bad and check([0, 1], [0], None, 1, n_links=1) == bad
    for kw in (dict(n_out=-1), dict(n_links=-1)):
        assert check([0, 0], [], [], 1, **kw) == bad and "negative" in _native.last_error()
    assert check([0, 0], [], [], -1) == bad


# ------------------------------------------------------------------------------------------------ the Python layer

def test_csr_keeps_the_order_of_a_rows_links_and_rounds_float_gains():
    links = [(2, 5, 1.0), (0, 1, 0.5), (2, 3, U), (0, 0, -1.0), (2, 5, 0.25), (0, 1, 1)]
    rp, ls, lg = live.medium_csr(3, links)
    assert rp.tolist() == [0, 3, 3, 6] and ls.tolist() == [1, 0, 1, 5, 3, 5]
    assert lg.tolist() == [U // 2, -U, 1, U, U, U // 4]
    assert all(a.dtype == np.int32 for a in (rp, ls, lg))
    assert live.medium_gain_q15(0.55) == round(0.55 * 32768) == 18022 and live.medium_gain_q15(18100) == 18100
    assert live.medium_gain_q15(np.float32(2.0)) == 65536 and live.medium_gain_q15(np.int64(-3)) == -3
    for bad in ((3, 0, U), (-1, 0, U)):
        with pytest.raises(ValueError):
            live.medium_csr(3, [bad])
    with pytest.raises(TypeError):
        live.medium_gain_q15(True)


def test_from_matrix_expands_a_station_matrix_over_the_channels():
    # A - B - C: A and C both reach B but not each other, and nobody hears itself
    gain = [[0, 1.0, 0], [0.5, 0, 0.25], [0, 1.0, 0]]
    P = 3
    n_src, n_out, links = live.medium_matrix_links(gain, P)
    assert (n_src, n_out) == (9, 9) and len(links) == 4 * P
    q = (np.asarray(gain) * U).astype(int)
    dense = np.zeros((n_out, n_src), int)
    for o, s, g in links:
        assert dense[o, s] == 0
        dense[o, s] = g
    for l in range(3):
        for s in range(3):
            block = dense[l * P:(l + 1) * P, s * P:(s + 1) * P]
            assert (block == np.eye(P, dtype=int) * q[l, s]).all(), (l, s)
    assert [o for o, _, _ in links] == sorted(o for o, _, _ in links)
    # extra rows: every listener hears them, channel by channel
    n_src, n_out, links = live.medium_matrix_links(gain, P, extra=1)
    assert (n_src, n_out) == (12, 9) and len(links) == 4 * P + 3 * P
    assert all((l * P + c, 9 + c, U) in links for l in range(3) for c in range(P))
    n_src, n_out, links = live.medium_matrix_links([[1, 1]], 2, extra=(0.5, 2 * U - 1))
    assert (n_src, n_out) == (8, 2)
    assert links == [(0, 0, 1), (0, 2, 1), (0, 4, U // 2), (0, 6, 65535), (1, 1, 1), (1, 3, 1), (1, 5, U // 2),
                     (1, 7, 65535)]                              # (an int entry is Q15 already)
    # a rectangular matrix: two listeners, three stations
    n_src, n_out, links = live.medium_matrix_links([[1.0, 0, 1.0], [0, 1.0, 1.0]], 1)
    assert (n_src, n_out, links) == (3, 2, [(0, 0, U), (0, 2, U), (1, 1, U), (1, 2, U)])
    for bad in ([], [1.0, 2.0], [[]]):
        with pytest.raises(ValueError):
            live.medium_matrix_links(bad, 2)
    with pytest.raises(ValueError):
        live.medium_matrix_links([[1.0]], 0)


def test_a_medium_checks_its_links_before_it_needs_a_device():
    with pytest.raises(_native.AfskNativeError, match="names source 4"):
        live.LiveMedium(4, 2, [(0, 4, U)])
    with pytest.raises(_native.AfskNativeError, match="gain"):
        live.LiveMedium(4, 2, [(0, 1, 2.5)])
    with pytest.raises(ValueError):
        live.LiveMedium(4, 2, [(2, 1, U)])
    with pytest.raises(ValueError):
        live.LiveMedium(4, 2, [], noise_scale_q24=[1, 2, 3])
    with pytest.raises(TypeError):
        live.LiveMedium(4, 2, [], noise_scale_q24=[0.5, 0.5])
    with pytest.raises(ValueError):
        live.LiveMedium(4, 2, [], seed=2 ** 32)
    if _native.device_count() <= 0:
        with pytest.raises(_native.AfskNativeError, match="no HIP device"):
            live.LiveMedium(4, 2, [(0, 1, U)])


# ---------------------------------------------------------------------------------- the model at the header's limits

def test_the_model_at_32768_links_reaches_the_header_limit_and_clips():
    """The tables tests/test_gpu_live_mix.py mixes on the device, through the model at a few columns: a row of 32768
    links at -65535 on -32768 sums to 2147450880 -- the model asserts every partial sum below 2^31 -- and clips; the
    balanced row comes back to its unity source."""
    n_src, n_out, links = M.limit_links()
    row_ptr, link_src, gain = live.medium_csr(n_out, links)
    assert np.diff(row_ptr).tolist() == [M.MAX_DEGREE, M.MAX_DEGREE]
    assert M.MAX_DEGREE * ((-M.MAX_GAIN * -32768) >> 15) == 2147450880 == 2 ** 31 - 32768
    assert (M.MAX_DEGREE // 2 - 1) * ((-M.MAX_GAIN * -32768) >> 15) == 1073659905
    rng = np.random.default_rng(12)
    src = np.stack([np.full(5, -32768, np.int16), rng.integers(-32768, 32768, 5, dtype=np.int16)])
    got = M.mix(src, row_ptr, link_src, gain, n_out, 5)
    assert (got[0] == 32767).all() and (got[1] == src[1]).all()


def test_the_model_counts_the_first_32768_links_of_a_longer_span():
    n_src, n_out, links = M.span_links()
    row_ptr, link_src, gain = live.medium_csr(n_out, links)
    n = link_src.size
    assert row_ptr.tolist() == [0, M.MAX_DEGREE, n] and n == M.MAX_DEGREE + M.SPAN_TAIL > 40000
    rng = np.random.default_rng(13)
    src = rng.integers(-32768, 32768, (n_src, 6), dtype=np.int16)
    src[3] = np.array([4, -4, 400, -400, 32767, -32768])          # a quarter of it is never 0
    for span in (M.MAX_DEGREE, M.MAX_DEGREE + 1, 40000):
        got = M.mix(src, [0, span, n], link_src, gain, n_out, 6)
        assert (got[0] == src[1]).all(), span                     # row 0: its first 32768 links and no more
        tail = (n - span) * ((M.UNITY // 4 * src[3].astype(np.int64)) >> 15)
        assert (got[1] == np.clip(tail, -32768, 32767)).all(), span
    # the clamp is what keeps source 3 out of row 0: one more link would be heard
    assert (((M.UNITY // 4) * src[3].astype(np.int64)) >> 15 != 0).all()
