"""``afsk_live_mix_delayed`` through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's name
instead of running): a mix is exactly live_mix_delay_kernel, live_mix_history_kernel and live_mix_advance_kernel, in that
order; nothing at ``n_samples == 0`` or ``n_out == 0``; the mix's grid is ``n_out * ceil(T / 2048)`` and the history's
``n_src * ceil(min(T, hist_len) / 2048)``; and every refusal -- afsk_live_mix's, a bad ``hist_len``, a missing position,
history or delay array, a history that overlaps ``src`` or ``out``, a grid above 2^31 - 1 -- launches nothing and names
the entry."""
import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import last_error, launches_decoded

BAD = _native.E_INVALID_ARG
U = 32768
MIX, HISTORY, ADVANCE = "live_mix_delay_kernel", "live_mix_history_kernel", "live_mix_advance_kernel"
ALL = [MIX, HISTORY, ADVANCE]


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_delay", [_native.LIVE_DELAY_SIGNATURES])


class Args:
    """Host memory standing in for the device arrays of a delayed mix: n_src source rows and n_out output rows of
    ``width`` samples in ONE buffer (the sources first), the history [n_src, hist_len] in a buffer of its own (with room
    for one more row), every output row hearing ``degree`` sources."""

    def __init__(self, n_src=6, n_out=4, width=5000, degree=2, hist_len=4096):
        self.n_src, self.n_out, self.width, self.hist_len = n_src, n_out, width, hist_len
        self.buf = np.zeros((n_src + n_out, width), np.int16)
        self.hist = np.zeros((n_src + 1, hist_len), np.int16)
        self.row_ptr = (np.arange(n_out + 1) * degree).astype(np.int32)
        self.link_src = (np.arange(n_out * degree) % max(n_src, 1)).astype(np.int32)
        self.link_gain = np.full(n_out * degree, U, np.int32)
        self.link_delay = (np.arange(n_out * degree) % 5).astype(np.int32)
        self.lens = np.full(max(n_src, 1), width, np.int32)
        self.scale = np.full(max(n_out, 1), 1 << 20, np.int32)
        self.pos = np.zeros(1, np.int64)

    def at(self, row, col=0):
        return self.buf.ctypes.data + 2 * (row * self.width + col)

    def call(self, T=None, lens=False, noise=False, **kw):
        a = dict(src=self.at(0), src_stride=self.width, n_src=self.n_src, lens=self.lens.ctypes.data if lens else None,
                 row_ptr=self.row_ptr.ctypes.data, link_src=self.link_src.ctypes.data,
                 link_gain=self.link_gain.ctypes.data, link_delay=self.link_delay.ctypes.data,
                 n_links=self.link_src.size, out=self.at(self.n_src), out_stride=self.width, n_out=self.n_out,
                 T=self.width if T is None else T, scale=self.scale.ctypes.data if noise else None, seed=3, base=7,
                 pos=self.pos.ctypes.data, history=self.hist.ctypes.data, hist_len=self.hist_len, stream=None)
        a.update(kw)
        return list(a.values())


def test_a_mix_is_three_launches_in_order(stub):
    a = Args()
    launches_decoded(stub)
    far = dict(T=1 << 20, src_stride=1 << 20, out_stride=1 << 20, out=a.at(0) + 2 * 6 * (1 << 20),
               history=a.at(0) + 2 * 20 * (1 << 20))                                                  # (never touched)
    for kw in (dict(), dict(lens=True), dict(noise=True), dict(lens=True, noise=True), dict(T=1), dict(T=4096),
               dict(hist_len=8, T=5), dict(hist_len=8, T=8), dict(hist_len=8, T=24), far):
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == ALL, kw
        assert stub_lib.last_kernel(stub)[2] == 1                           # the advance: one block
    assert a.pos[0] == 0 and not a.buf.any() and not a.hist.any()           # (the stub runs no kernel)


def test_nothing_to_write_launches_nothing(stub):
    a = Args()
    launches_decoded(stub)
    for kw in (dict(T=0), dict(T=0, noise=True), dict(n_out=0), dict(n_out=0, out=None, row_ptr=None),
               dict(T=0, src=None, n_src=0, history=None)):
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == 0, (kw, last_error(stub))
    assert launches_decoded(stub) == [] and a.pos[0] == 0
    # no sources, no links: the rows are zeroed and the position advances; there is no history to write
    assert stub.afsk_live_mix_delayed(*a.call(n_src=0, src=None, history=None, n_links=0, link_src=None, link_gain=None,
                                              link_delay=None)) == 0, last_error(stub)
    assert launches_decoded(stub) == [MIX, ADVANCE]


# ------------------------------------------------------------------------------------------------------- the grids
# The stub keeps the grid of the LAST launch only, and the last launch of a delayed mix is the advance.  Both grids are
# checked against 2^31 - 1 before anything is launched, so the formulas show at that edge: a shape whose grid is exactly
# 2^31 - 1 (or the largest the formula can give below it) is launched, the next one is refused, and the refusal says
# which grid it was.  (Rows that far apart are never touched: the stub runs no kernel.)

SRC, OUT, HIST = 1 << 12, 1 << 56, 1 << 60                      # byte addresses with 2^51 bytes and more between them
M31 = 2 ** 31 - 1


def huge(stub, a, n_src, n_out, T, hist_len):
    kw = dict(src=SRC, out=OUT, history=HIST, src_stride=1 << 20, out_stride=1 << 20, n_src=n_src, n_out=n_out, T=T,
              hist_len=hist_len)
    return stub.afsk_live_mix_delayed(*a.call(**kw))


@pytest.mark.parametrize("T,tiles", [(1, 1), (2047, 1), (2048, 1), (2049, 2), (4096, 2), (4097, 3), (6000, 3),
                                     (1 << 20, 512)])
def test_the_mix_grid_is_rows_times_tiles(stub, T, tiles):
    """n_out * ceil(T / 2048): the largest n_out with n_out * tiles <= 2^31 - 1 is launched, one more row is refused."""
    a = Args()
    launches_decoded(stub)
    most = M31 // tiles
    assert huge(stub, a, 1, most, T, 8) == 0, last_error(stub)
    assert launches_decoded(stub) == ALL
    if most < M31:
        assert huge(stub, a, 1, most + 1, T, 8) == BAD
        assert "afsk_live_mix_delayed" in last_error(stub) and "n_out * tiles" in last_error(stub)
        assert launches_decoded(stub) == []


@pytest.mark.parametrize("T,hist_len,tiles", [(1, 8, 1), (8, 8, 1), (24, 8, 1), (1 << 20, 8, 1), (2048, 2048, 1),
                                              (2049, 2048, 1), (2048, 4096, 1), (2049, 4096, 2), (4096, 4096, 2),
                                              (6000, 4096, 2), (6000, 8192, 3), (1 << 20, 1 << 19, 256),
                                              (1 << 20, 1 << 20, 512), (5000, 1 << 20, 3)])
def test_the_history_grid_is_sources_times_tiles_of_what_it_writes(stub, T, hist_len, tiles):
    """n_src * ceil(min(T, hist_len) / 2048), at the same edge; one output row keeps the mix's grid small."""
    a = Args()
    launches_decoded(stub)
    assert tiles == -(-min(T, hist_len) // 2048)
    most = M31 // tiles
    assert huge(stub, a, most, 1, T, hist_len) == 0, last_error(stub)
    assert launches_decoded(stub) == ALL
    if most < M31:
        assert huge(stub, a, most + 1, 1, T, hist_len) == BAD
        assert "afsk_live_mix_delayed" in last_error(stub) and "history" in last_error(stub) and "2^31" in last_error(stub)
        assert launches_decoded(stub) == []


# ---------------------------------------------------------------------------------------------------- the refusals

def test_refusals_launch_nothing_and_name_the_entry(stub):
    a = Args()
    launches_decoded(stub)
    cases = [(dict(src=None), "null"), (dict(out=None), "null"), (dict(row_ptr=None), "null"),
             (dict(link_src=None), "null"), (dict(link_gain=None), "null"),
             (dict(link_delay=None), "null"), (dict(pos=None), "null"), (dict(history=None), "null"),
             (dict(pos=None, T=0), "null"), (dict(history=None, n_out=0), "null"),
             (dict(n_src=-1), "negative"), (dict(n_out=-1), "negative"), (dict(n_links=-1), "negative"),
             (dict(T=-1), "n_samples"), (dict(T=(1 << 20) + 1), "n_samples"),
             (dict(src_stride=a.width - 1), "stride"), (dict(out_stride=a.width - 1), "stride"),
             (dict(src_stride=-a.width), "stride"), (dict(out_stride=0), "stride")]
    cases += [(dict(hist_len=h), "hist_len") for h in (0, -8, 1, 4, 7, 9, 12, 4095, 4097, (1 << 20) + 1, 1 << 21,
                                                        2 ** 31 - 1, -2 ** 31)]
    for kw, word in cases:
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == BAD, kw
        assert "afsk_live_mix_delayed" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
        assert launches_decoded(stub) == [], kw
    # with one row its stride is not looked at; with no links the link arrays may be NULL; without sources no history
    one = Args(n_src=1, n_out=1, degree=1)
    assert stub.afsk_live_mix_delayed(*one.call(src_stride=0, out_stride=-5)) == 0, last_error(stub)
    assert stub.afsk_live_mix_delayed(*a.call(n_links=0, link_src=None, link_gain=None, link_delay=None)) == 0
    assert launches_decoded(stub) == ALL + ALL
    for h in (8, 16, 1 << 20):
        big = Args(n_src=1, n_out=1, degree=1, width=64, hist_len=h)
        assert stub.afsk_live_mix_delayed(*big.call()) == 0, (h, last_error(stub))
        assert launches_decoded(stub) == ALL
    assert not a.buf.any() and a.pos[0] == 0 and not a.hist.any()


def test_out_must_not_overlap_src(stub):
    a = Args()                                                          # sources: rows 0 ... 5; outputs behind them
    T = a.width
    launches_decoded(stub)
    for kw in (dict(out=a.at(0)), dict(out=a.at(5)), dict(out=a.at(5, T - 1)), dict(out=a.at(2, 17)),
               dict(out=a.at(0), n_out=1), dict(src=a.at(3), out=a.at(0)),
               dict(src=a.at(4), n_src=2, out=a.at(0), n_out=4, T=T - 1, out_stride=T + 1)):
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == BAD, kw
        assert "afsk_live_mix_delayed" in last_error(stub) and "out overlaps src" in last_error(stub), kw
    assert launches_decoded(stub) == []
    for kw in (dict(out=a.at(6)), dict(src=a.at(4), n_src=2, out=a.at(0)), dict(T=100, out=a.at(5, 100), n_out=1),
               dict(T=100, src=a.at(0, 100), n_src=1, out=a.at(0), n_out=1)):
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == ALL, kw


def test_the_history_must_overlap_neither_src_nor_out(stub):
    """The history's bytes are [history, + 2 * n_src * hist_len); src's and out's run from the first row's first column
    to the last row's column T."""
    a = Args(hist_len=1024)                                             # 6 sources, 4 outputs, rows of 5000
    T, H = a.width, 2 * 6 * 1024                                        # (the history's bytes)
    launches_decoded(stub)
    src_end, out_end = a.at(6), a.at(10)
    for kw, word in ((dict(history=a.at(0)), "src"), (dict(history=a.at(5, T - 1)), "src"),
                     (dict(history=a.at(0) - H + 2), "src"),                       # its last sample is src's first
                     (dict(history=a.at(3, 40)), "src"),
                     (dict(history=a.at(6)), "out"), (dict(history=a.at(9, T - 1)), "out"),
                     (dict(history=a.at(8, 1)), "out"),
                     (dict(history=a.at(5, T - 1), n_out=0), "src"),                # no output rows: src still counts
                     (dict(history=a.at(0) - H + 2, n_src=1, hist_len=4096 + 2048), "hist_len")):
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == BAD, kw
        err = last_error(stub)
        assert "afsk_live_mix_delayed" in err and word in err and ("history overlaps" in err or word == "hist_len"), (kw, err)
    assert launches_decoded(stub) == []
    # touching ranges do not overlap: the history right behind out's last column, or ending right in front of src
    for kw in (dict(history=out_end), dict(history=a.at(0) - H), dict(history=a.hist.ctypes.data),
               dict(T=100, history=a.at(9, 100)),                                   # behind column T of the last row
               dict(n_src=1, out=a.at(6), history=a.at(0, T))):                     # one source: only ITS row counts
        assert stub.afsk_live_mix_delayed(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == ALL, kw
    assert src_end == a.at(a.n_src)
