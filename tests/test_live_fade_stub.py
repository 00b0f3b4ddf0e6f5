"""``afsk_live_mix_faded`` through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's name
instead of running): a faded mix is exactly live_mix_fade_kernel, live_mix_history_kernel and live_mix_advance_kernel, in
that order; nothing at ``n_samples == 0`` or ``n_out == 0``; the mix's grid is ``n_out * ceil(T / 2048)`` and the
history's ``n_src * ceil(min(T, hist_len) / 2048)``; every refusal -- the filtered entry's, and a missing fade array --
launches nothing and names the entry; and the filtered, the delayed and the undelayed entries launch what they launched."""
import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import last_error, launches_decoded

BAD = _native.E_INVALID_ARG
U = 32768
MIX, HISTORY, ADVANCE = "live_mix_fade_kernel", "live_mix_history_kernel", "live_mix_advance_kernel"
ALL = [MIX, HISTORY, ADVANCE]


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_fade", [_native.LIVE_FADE_SIGNATURES, _native.LIVE_FIR_SIGNATURES,
                                                              _native.LIVE_DELAY_SIGNATURES, _native.LIVE_MIX_SIGNATURES])


class Args:
    """Host memory standing in for the device arrays of a faded mix: tests/test_live_fir_stub.py's layout plus a track
    and an offset per link and a table of three tracks."""

    def __init__(self, n_src=6, n_out=4, width=5000, degree=2, hist_len=4096):
        self.n_src, self.n_out, self.width, self.hist_len = n_src, n_out, width, hist_len
        self.buf = np.zeros((n_src + n_out, width), np.int16)
        self.hist = np.zeros((n_src + 1, hist_len), np.int16)
        self.row_ptr = (np.arange(n_out + 1) * degree).astype(np.int32)
        self.link_src = (np.arange(n_out * degree) % max(n_src, 1)).astype(np.int32)
        self.link_gain = np.full(n_out * degree, U, np.int32)
        self.link_delay = (np.arange(n_out * degree) % 5).astype(np.int32)
        self.link_filter = (np.arange(n_out * degree) % 4 - 1).astype(np.int32)
        self.filter_ptr = np.asarray([0, 1, 4, 8], np.int32)
        self.taps = np.asarray([16384, 1, 2, 3, 4, 5, 6, 7], np.int16)
        self.link_fade = (np.arange(n_out * degree) % 3 - 1).astype(np.int32)
        self.link_fade_offset = (np.arange(n_out * degree) * 0x9E3779B1).astype(np.uint32)
        self.fade_ptr = np.asarray([0, 1, 3, 7], np.int32)
        self.fade_shift = np.asarray([3, 9, 15], np.int32)
        self.knots = np.asarray([U, 0, 65535, 1, 2, 3, 4], np.uint16)
        self.lens = np.full(max(n_src, 1), width, np.int32)
        self.scale = np.full(max(n_out, 1), 1 << 20, np.int32)
        self.pos = np.zeros(1, np.int64)

    def at(self, row, col=0):
        return self.buf.ctypes.data + 2 * (row * self.width + col)

    def call(self, T=None, lens=False, noise=False, **kw):
        a = dict(src=self.at(0), src_stride=self.width, n_src=self.n_src, lens=self.lens.ctypes.data if lens else None,
                 row_ptr=self.row_ptr.ctypes.data, link_src=self.link_src.ctypes.data,
                 link_gain=self.link_gain.ctypes.data, link_delay=self.link_delay.ctypes.data,
                 link_filter=self.link_filter.ctypes.data, n_links=self.link_src.size, out=self.at(self.n_src),
                 out_stride=self.width, n_out=self.n_out, T=self.width if T is None else T,
                 scale=self.scale.ctypes.data if noise else None, seed=3, base=7, pos=self.pos.ctypes.data,
                 history=self.hist.ctypes.data, hist_len=self.hist_len, filter_ptr=self.filter_ptr.ctypes.data,
                 taps=self.taps.ctypes.data, n_filters=3, n_taps=8, link_fade=self.link_fade.ctypes.data,
                 link_fade_offset=self.link_fade_offset.ctypes.data, fade_ptr=self.fade_ptr.ctypes.data,
                 fade_shift=self.fade_shift.ctypes.data, knots=self.knots.ctypes.data, n_fades=3, n_knots=7, stream=None)
        a.update(kw)
        return list(a.values())

    def filtered(self, **kw):
        a = self.call(**kw)
        return a[:24] + a[31:]

    def delayed(self, **kw):
        a = self.filtered(**kw)
        return a[:8] + a[9:20] + a[24:]

    def plain(self, **kw):
        a = self.filtered(**kw)
        return a[:7] + a[9:18] + a[24:]


def test_a_faded_mix_is_three_launches_in_order(stub):
    a = Args()
    launches_decoded(stub)
    far = dict(T=1 << 20, src_stride=1 << 20, out_stride=1 << 20, out=a.at(0) + 2 * 6 * (1 << 20),
               history=a.at(0) + 2 * 20 * (1 << 20))                                                  # (never touched)
    for kw in (dict(), dict(lens=True), dict(noise=True), dict(lens=True, noise=True), dict(T=1), dict(T=4096),
               dict(hist_len=8, T=5), dict(hist_len=8, T=8), dict(hist_len=8, T=24), dict(n_filters=0, n_taps=0, taps=None),
               dict(n_fades=0, n_knots=0, knots=None, fade_shift=None), far):
        assert stub.afsk_live_mix_faded(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == ALL, kw
        assert stub_lib.last_kernel(stub)[2] == 1                           # the advance: one block
    assert a.pos[0] == 0 and not a.buf.any() and not a.hist.any()           # (the stub runs no kernel)


def test_nothing_to_write_launches_nothing(stub):
    a = Args()
    launches_decoded(stub)
    for kw in (dict(T=0), dict(T=0, noise=True), dict(n_out=0), dict(n_out=0, out=None, row_ptr=None),
               dict(T=0, src=None, n_src=0, history=None)):
        assert stub.afsk_live_mix_faded(*a.call(**kw)) == 0, (kw, last_error(stub))
    assert launches_decoded(stub) == [] and a.pos[0] == 0
    # no sources, no links: the rows are zeroed and the position advances; there is no history to write
    assert stub.afsk_live_mix_faded(*a.call(n_src=0, src=None, history=None, n_links=0, link_src=None, link_gain=None,
                                            link_delay=None, link_filter=None, link_fade=None,
                                            link_fade_offset=None)) == 0, last_error(stub)
    assert launches_decoded(stub) == [MIX, ADVANCE]


# The stub keeps the grid of the LAST launch only (the advance), so both grids show at the 2^31 - 1 refusal edge, as in
# tests/test_live_delay_stub.py: the largest shape is launched, the next one refused, and the refusal says which grid.

SRC, OUT, HIST = 1 << 12, 1 << 56, 1 << 60                      # byte addresses with 2^51 bytes and more between them
M31 = 2 ** 31 - 1


def huge(stub, a, n_src, n_out, T, hist_len):
    kw = dict(src=SRC, out=OUT, history=HIST, src_stride=1 << 20, out_stride=1 << 20, n_src=n_src, n_out=n_out, T=T,
              hist_len=hist_len)
    return stub.afsk_live_mix_faded(*a.call(**kw))


@pytest.mark.parametrize("T,tiles", [(1, 1), (2047, 1), (2048, 1), (2049, 2), (4097, 3), (1 << 20, 512)])
def test_the_mix_grid_is_rows_times_tiles(stub, T, tiles):
    a = Args()
    launches_decoded(stub)
    most = M31 // tiles
    assert huge(stub, a, 1, most, T, 8) == 0, last_error(stub)
    assert launches_decoded(stub) == ALL
    if most < M31:
        assert huge(stub, a, 1, most + 1, T, 8) == BAD
        assert "afsk_live_mix_faded" in last_error(stub) and "n_out * tiles" in last_error(stub)
        assert launches_decoded(stub) == []


@pytest.mark.parametrize("T,hist_len,tiles", [(24, 8, 1), (1 << 20, 8, 1), (2049, 2048, 1), (2049, 4096, 2),
                                              (6000, 4096, 2), (6000, 8192, 3), (1 << 20, 1 << 20, 512)])
def test_the_history_grid_is_sources_times_tiles_of_what_it_writes(stub, T, hist_len, tiles):
    a = Args()
    launches_decoded(stub)
    assert tiles == -(-min(T, hist_len) // 2048)
    most = M31 // tiles
    assert huge(stub, a, most, 1, T, hist_len) == 0, last_error(stub)
    assert launches_decoded(stub) == ALL
    if most < M31:
        assert huge(stub, a, most + 1, 1, T, hist_len) == BAD
        assert "afsk_live_mix_faded" in last_error(stub) and "history" in last_error(stub) and "2^31" in last_error(stub)
        assert launches_decoded(stub) == []


def test_refusals_launch_nothing_and_name_the_entry(stub):
    a = Args()
    launches_decoded(stub)
    cases = [(dict(src=None), "null"), (dict(out=None), "null"), (dict(row_ptr=None), "null"),
             (dict(link_src=None), "null"), (dict(link_gain=None), "null"), (dict(link_delay=None), "null"),
             (dict(link_filter=None), "null"), (dict(filter_ptr=None), "null"), (dict(taps=None), "null"),
             (dict(filter_ptr=None, n_filters=0, n_taps=0), "null"),
             (dict(link_fade=None), "null"), (dict(link_fade_offset=None), "null"), (dict(fade_ptr=None), "null"),
             (dict(fade_shift=None), "null"), (dict(knots=None), "null"),
             (dict(fade_ptr=None, n_fades=0, n_knots=0), "null"), (dict(fade_ptr=None, T=0), "null"),
             (dict(knots=None, n_out=0), "null"),
             (dict(pos=None), "null"), (dict(history=None), "null"), (dict(pos=None, T=0), "null"),
             (dict(filter_ptr=None, T=0), "null"), (dict(history=None, n_out=0), "null"),
             (dict(n_src=-1), "negative"), (dict(n_out=-1), "negative"), (dict(n_links=-1), "negative"),
             (dict(n_filters=-1), "negative"), (dict(n_taps=-1), "negative"),
             (dict(n_fades=-1), "negative"), (dict(n_knots=-1), "negative"),
             (dict(T=-1), "n_samples"), (dict(T=(1 << 20) + 1), "n_samples"),
             (dict(src_stride=a.width - 1), "stride"), (dict(out_stride=a.width - 1), "stride"),
             (dict(src_stride=-a.width), "stride"), (dict(out_stride=0), "stride"),
             (dict(out=a.at(0)), "out overlaps src"), (dict(out=a.at(5, a.width - 1)), "out overlaps src"),
             (dict(history=a.at(0)), "history overlaps src"), (dict(history=a.at(9, a.width - 1)), "history overlaps out")]
    cases += [(dict(hist_len=h), "hist_len") for h in (0, -8, 1, 4, 7, 9, 12, 4095, (1 << 20) + 1, 2 ** 31 - 1, -2 ** 31)]
    for kw, word in cases:
        assert stub.afsk_live_mix_faded(*a.call(**kw)) == BAD, kw
        assert "afsk_live_mix_faded" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
        assert launches_decoded(stub) == [], kw
    # with no links the link arrays may be NULL; with no taps the tap array; with no knots the knots and, with no tracks,
    # the shifts; touching ranges do not overlap
    assert stub.afsk_live_mix_faded(*a.call(n_links=0, link_src=None, link_gain=None, link_delay=None, link_filter=None,
                                            link_fade=None, link_fade_offset=None)) == 0, last_error(stub)
    assert stub.afsk_live_mix_faded(*a.call(n_taps=0, taps=None)) == 0, last_error(stub)
    assert stub.afsk_live_mix_faded(*a.call(n_knots=0, knots=None)) == 0, last_error(stub)
    assert stub.afsk_live_mix_faded(*a.call(n_fades=0, fade_shift=None)) == 0, last_error(stub)
    assert stub.afsk_live_mix_faded(*a.call(history=a.at(10))) == 0, last_error(stub)
    assert launches_decoded(stub) == ALL * 5
    assert not a.buf.any() and a.pos[0] == 0 and not a.hist.any()


def test_the_earlier_entries_launch_what_they_launched(stub):
    a = Args()
    launches_decoded(stub)
    assert stub.afsk_live_mix_filtered(*a.filtered()) == 0, last_error(stub)
    assert launches_decoded(stub) == ["live_mix_fir_kernel", HISTORY, ADVANCE]
    assert stub.afsk_live_mix_delayed(*a.delayed()) == 0, last_error(stub)
    assert launches_decoded(stub) == ["live_mix_delay_kernel", HISTORY, ADVANCE]
    assert stub.afsk_live_mix(*a.plain()) == 0, last_error(stub)
    assert launches_decoded(stub) == ["live_mix_kernel", ADVANCE]
    assert stub.afsk_live_mix(*a.plain(pos=None)) == 0, last_error(stub)
    assert launches_decoded(stub) == ["live_mix_kernel"]
