"""``afsk_live_mix`` through the stub HIP runtime (no GPU; tests/stub_lib.py: a launch records the kernel's name instead
of running): a mix is one launch of live_mix_kernel, two -- live_mix_advance_kernel behind it -- when a position is
kept, none at ``n_samples == 0`` or ``n_out == 0``; the grid is ``n_out * ceil(T / 2048)``; and every refusal, the
overlap of ``out`` and ``src`` among them, launches nothing and names the entry."""
import numpy as np
import pytest

from afskmodem_amd import _native
from tests import stub_lib
from tests.stub_lib import last_error, last_kernel, launches_decoded

BAD = _native.E_INVALID_ARG
U = 32768
MIX, ADVANCE = "live_mix_kernel", "live_mix_advance_kernel"


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return stub_lib.load(tmp_path_factory, "afsk_stub_mix", [_native.LIVE_MIX_SIGNATURES])


class Args:
    """Host memory standing in for the device arrays of a mix: n_src source rows and n_out output rows of ``width``
    samples in ONE buffer (the sources first), every output row hearing ``degree`` sources."""

    def __init__(self, n_src=6, n_out=4, width=5000, degree=2):
        self.n_src, self.n_out, self.width = n_src, n_out, width
        self.buf = np.zeros((n_src + n_out, width), np.int16)
        self.row_ptr = (np.arange(n_out + 1) * degree).astype(np.int32)
        self.link_src = (np.arange(n_out * degree) % max(n_src, 1)).astype(np.int32)
        self.link_gain = np.full(n_out * degree, U, np.int32)
        self.lens = np.full(max(n_src, 1), width, np.int32)
        self.scale = np.full(max(n_out, 1), 1 << 20, np.int32)
        self.pos = np.zeros(1, np.int64)

    def at(self, row, col=0):
        return self.buf.ctypes.data + 2 * (row * self.width + col)

    def call(self, T=None, lens=False, noise=False, pos=False, **kw):
        a = dict(src=self.at(0), src_stride=self.width, n_src=self.n_src, lens=self.lens.ctypes.data if lens else None,
                 row_ptr=self.row_ptr.ctypes.data, link_src=self.link_src.ctypes.data,
                 link_gain=self.link_gain.ctypes.data, n_links=self.link_src.size, out=self.at(self.n_src),
                 out_stride=self.width, n_out=self.n_out, T=self.width if T is None else T,
                 scale=self.scale.ctypes.data if noise else None, seed=3, base=7,
                 pos=self.pos.ctypes.data if pos else None, stream=None)
        a.update(kw)
        return list(a.values())


def test_a_mix_is_one_launch_and_two_with_a_position(stub):
    a = Args()
    launches_decoded(stub)
    far = dict(T=1 << 20, src_stride=1 << 20, out_stride=1 << 20, out=a.at(0) + 2 * 6 * (1 << 20))    # (never touched)
    for kw in (dict(), dict(lens=True), dict(noise=True), dict(lens=True, noise=True), dict(T=1), far):
        assert stub.afsk_live_mix(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == [MIX], kw
    for kw in (dict(pos=True), dict(pos=True, noise=True), dict(pos=True, noise=True, lens=True)):
        assert stub.afsk_live_mix(*a.call(**kw)) == 0, kw
        assert launches_decoded(stub) == [MIX, ADVANCE], kw
        assert last_kernel(stub)[2] == 1                                # the advance: one block
    assert a.pos[0] == 0 and not a.buf.any()                            # (the stub runs no kernel)


def test_nothing_to_write_launches_nothing(stub):
    a = Args()
    launches_decoded(stub)
    for kw in (dict(T=0), dict(T=0, pos=True, noise=True), dict(n_out=0), dict(n_out=0, out=None, row_ptr=None, pos=True),
               dict(T=0, src=None, n_src=0)):
        assert stub.afsk_live_mix(*a.call(**kw)) == 0, (kw, last_error(stub))
    assert launches_decoded(stub) == [] and a.pos[0] == 0
    # no sources, no links: a launch all the same (the rows are zeroed)
    assert stub.afsk_live_mix(*a.call(n_src=0, src=None, n_links=0, link_src=None, link_gain=None)) == 0
    assert launches_decoded(stub) == [MIX]


@pytest.mark.parametrize("n_out,T,grid", [(4, 1, 4), (4, 2048, 4), (4, 2049, 8), (3, 5000, 9), (70000, 8, 70000),
                                          (1, 1 << 20, 512), (4194303, 1 << 20, 2 ** 31 - 512)])
def test_the_grid_is_rows_times_tiles(stub, n_out, T, grid):
    a = Args()
    big = dict(n_out=n_out, T=T, src_stride=1 << 20, out_stride=1 << 20, n_src=1, out=a.at(0) + (1 << 22))
    assert stub.afsk_live_mix(*a.call(**big)) == 0, last_error(stub)
    n, name, got = last_kernel(stub)
    assert MIX in name and got == grid
    launches_decoded(stub)


def test_a_grid_above_2_31_is_refused(stub):
    a = Args()
    launches_decoded(stub)
    big = dict(T=1 << 20, src_stride=1 << 20, out_stride=1 << 20, n_src=1, out=a.at(0) + (1 << 22))
    assert stub.afsk_live_mix(*a.call(n_out=4194304, **big)) == BAD     # 2^22 rows * 512 tiles = 2^31
    assert "afsk_live_mix" in last_error(stub) and "2^31" in last_error(stub)
    assert launches_decoded(stub) == []


def test_refusals_launch_nothing_and_name_the_entry(stub):
    a = Args()
    launches_decoded(stub)
    cases = [(dict(src=None), "null"), (dict(out=None), "null"), (dict(row_ptr=None), "null"),
             (dict(link_src=None), "null"), (dict(link_gain=None), "null"),
             (dict(n_src=-1), "negative"), (dict(n_out=-1), "negative"), (dict(n_links=-1), "negative"),
             (dict(T=-1), "n_samples"), (dict(T=(1 << 20) + 1), "n_samples"),
             (dict(src_stride=a.width - 1), "stride"), (dict(out_stride=a.width - 1), "stride"),
             (dict(src_stride=-a.width), "stride"), (dict(out_stride=0), "stride")]
    for kw, word in cases:
        assert stub.afsk_live_mix(*a.call(**kw)) == BAD, kw
        assert "afsk_live_mix" in last_error(stub) and word in last_error(stub), (kw, last_error(stub))
    # with one row its stride is not looked at; with no links the link arrays may be NULL
    one = Args(n_src=1, n_out=1, degree=1)
    assert stub.afsk_live_mix(*one.call(src_stride=0, out_stride=-5)) == 0, last_error(stub)
    assert stub.afsk_live_mix(*a.call(n_links=0, link_src=None, link_gain=None)) == 0
    assert launches_decoded(stub) == [MIX, MIX]
    assert not a.buf.any() and a.pos[0] == 0


def test_out_must_not_overlap_src(stub):
    a = Args()                                                          # sources: rows 0 ... 5; outputs behind them
    T = a.width
    launches_decoded(stub)
    overlapping = [dict(out=a.at(0)), dict(out=a.at(5)), dict(out=a.at(5, T - 1)), dict(out=a.at(2, 17)),
                   dict(out=a.at(0), n_out=1), dict(src=a.at(3), out=a.at(0)),         # out in front, reaching in
                   dict(src=a.at(4), n_src=2, out=a.at(0), n_out=4, T=T - 1, out_stride=T + 1)]
    for kw in overlapping:
        assert stub.afsk_live_mix(*a.call(**kw)) == BAD, kw
        assert "afsk_live_mix" in last_error(stub) and "overlap" in last_error(stub), kw
    assert launches_decoded(stub) == []
    # touching ranges do not overlap: out right behind the last source column, or ending right in front of the first
    for kw in (dict(out=a.at(6)), dict(src=a.at(4), n_src=2, out=a.at(0)), dict(T=100, out=a.at(5, 100), n_out=1),
               dict(T=100, src=a.at(0, 100), n_src=1, out=a.at(0), n_out=1),
               dict(n_src=0, src=None, out=a.at(0))):           # no sources: nothing to overlap
        assert stub.afsk_live_mix(*a.call(**kw)) == 0, (kw, last_error(stub))
        assert launches_decoded(stub) == [MIX], kw
