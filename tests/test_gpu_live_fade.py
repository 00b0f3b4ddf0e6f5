"""GPU parity (-m gpu) of the faded live medium: ``LiveMedium(fades=)`` (afsk_live_mix_faded: live_mix_fade_kernel,
live_mix_history_kernel, live_mix_advance_kernel) against the numpy model over an explicit timeline
(tests/live_fade_model.py), sample for sample.

Expected values never come from the code under test: the mix is the model's (one whole signal per source, no ring, the
rule in int64 with the int32 fits asserted), its noise the CPU oracle's generator.  Two tests hold the device against
itself where the header says two things are equal (a unity track against afsk_live_mix_filtered, a captured graph against
eager), and both sides against the model.  The last test holds the medium against existing pieces: a LiveTransmitter's
two messages through one faded link into a streaming LiveReceiver, whose bursts must be what the oracle's gate and
decoder report on the MODEL's rows.  Integer samples: every comparison is exact.  Shapes stay small (n_src <= 6,
n_out <= 4, T <= 4200 per mix, one check mix of a sum above that): the shifts, the offsets, T and the start sit at the
edges of the kernel's paths -- a knot boundary at each of a thread's 8 columns, the track's end, the 2048-column tile,
the ring's end, 2^32."""
import numpy as np
import pytest

from afskmodem_amd import _native, live
from afskmodem_amd.live import LiveMedium, LiveReceiver, LiveTransmitter
from tests import live_fade_model as FD
from tests import live_mix_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import collect
from tests.live_drive import same as same_bursts
from tests.test_gpu_live_mix import same, strided, upload
from tests.test_gpu_live_stream import expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = M.UNITY
Q14 = 16384
POISON = 32767


def tables_of(medium):
    """The link, filter and fade tables as they lie ON THE DEVICE now."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(row_ptr=host(medium.d_row_ptr), link_src=host(medium.d_link_src), link_gain_q15=host(medium.d_link_gain_q15),
                link_delay=host(medium.d_link_delay), link_filter=host(medium.d_link_filter),
                filter_ptr=host(medium.d_filter_ptr), filter_taps=host(medium.d_filter_taps),
                link_fade=host(medium.d_link_fade), link_fade_offset=host(medium.d_link_fade_offset),
                fade_ptr=host(medium.d_fade_ptr), fade_shift=host(medium.d_fade_shift),
                fade_knots=host(medium.d_fade_knots))


def expect(tl, medium, src, T, lens=None):
    """The model's next mix over the device's tables; ``tl``: the ``FD.Timeline`` that follows ``medium``."""
    scale = None if medium.d_noise_scale_q24 is None else medium.d_noise_scale_q24.cpu().numpy()
    return tl.mix(src, n_out=medium.n_out, T=T, src_lens=lens, noise_scale_q24=scale, seed=medium.seed,
                  noise_idx_base=medium.noise_idx_base, **tables_of(medium))


def timeline(medium, pos=0):
    return FD.Timeline(medium.n_src, medium.hist_len, pos)


def random_taps(rng, K):
    """K taps whose magnitudes sum to at most 65535, the first and the last not 0."""
    top = min(32767, 65535 // K)
    h = rng.integers(-top, top + 1, K)
    h[0], h[-1] = top, -top
    return [int(t) for t in h]


def random_knots(rng, L):
    """L knots over the whole range, with both ends of it among them when there is room."""
    k = rng.integers(0, 65536, L)
    if L >= 4:
        k[0], k[1], k[-1] = 65535, 0, 1
    return [int(v) for v in k]


def run(torch, medium, tl, rng, Ts, lens=None, full=32768, tag=()):
    """Ticks of random sources through ``medium`` against the model; the last (got, want)."""
    for i, T in enumerate(Ts):
        host = rng.integers(-full, full, (medium.n_src, T + 3), dtype=np.int16)
        src, _ = strided(torch, medium.n_src, T, 1)
        upload(torch, host, src)
        out, flat = strided(torch, medium.n_out, T, 3, fill=POISON)
        got = medium.mix(src, T, out=out, lengths=lens)
        want = expect(tl, medium, host, T, lens)
        same(got, want, (*tag, i, T))
        rest = torch.ones_like(flat, dtype=torch.bool)
        rest.as_strided((medium.n_out, T), (T + 3, 1), 3).fill_(False)
        assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
    assert medium.pos == tl.pos
    return got, want


# ------------------------------------------------------------------------------------------------- 1. knot straddling

@pytest.mark.parametrize("L", [1, 2, 64])
@pytest.mark.parametrize("p", [3, 4, 11, 15])
def test_a_knot_boundary_at_every_column_of_a_thread_and_the_tracks_end(torch_cuda, p, L):
    """Eight links whose offsets are the track's length minus 0 ... 7: at medium time 0 link i is i samples before
    its track's end, so the boundary between the LAST knot and the first lies i columns into the first thread's 8 (0: at
    its first column), and with p = 3 or 4 every later thread has one there too.  Rows 2 and 3 take the staged filter
    path.  The second tick crosses the 2048-column tile."""
    torch = torch_cuda
    rng = np.random.default_rng(100 * p + L)
    period = L << p
    links = [(i // 2, i % 6, U // 2 if i % 3 else -U // 2, (0, 3, 9)[i % 3], 0 if i >= 4 else None, 0, period - i)
             for i in range(8)]
    medium = LiveMedium(6, 4, links, filters=[random_taps(rng, 17)], fades=[(random_knots(rng, L), 1 << p)], device=DEV)
    assert medium.faded and medium.filtered and medium.delayed and medium.hist_len == 32
    assert medium.n_fades == 1 and medium.fade_ptr.tolist() == [0, L] and medium.fade_shift.tolist() == [p]
    assert medium.fade_knots.dtype == np.uint16 and medium.link_fade_offset.tolist() == [period - i for i in range(8)]
    assert medium.d_fade_knots.dtype == torch.uint16 and medium.d_link_fade_offset.dtype == torch.uint32
    tl = timeline(medium)
    got, want = run(torch, medium, tl, rng, [5, 2049, 37], tag=(p, L))
    assert all(want[r].any() for r in range(4))


def test_a_medium_with_fades_and_nothing_else_is_delayed_with_the_smallest_history(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(1)
    medium = LiveMedium(2, 2, [(0, 0, U, 0, None, 0), (1, 1, U)], fades=[(random_knots(rng, 8), 16)], device=DEV)
    assert medium.faded and medium.delayed and not medium.filtered and medium.hist_len == 8 and medium.n_filters == 0
    plain = LiveMedium(2, 2, [(0, 0, U), (1, 1, U)], device=DEV)
    assert not plain.faded and plain.n_fades == 0 and plain.d_fade_knots is None and plain.d_link_fade is None
    assert not plain.delayed and plain.d_history is None and plain.d_link_filter is None       # allocates what it did
    got, want = run(torch, medium, timeline(medium), rng, [300, 9])
    assert want[0].any()


# ----------------------------------------------------------------------------------------------------- 2. knot values

def test_the_knot_values_at_both_ends_against_full_scale_samples(torch_cuda):
    """Constant tracks of 0, 1, 32767, 32768 and 65535 and one that runs between them, against sources that hold
    -32768 and 32767 among others: 65535 * -32768 >> 15 = -65535 is clamped to -32768 BEFORE the gain, so at gain 1/2
    the link gives -16384 (clamped behind the gain alone it would give -32768); a zero track leaves only the noise."""
    torch = torch_cuda
    rng = np.random.default_rng(2)
    fades = [([v], 8) for v in (0, 1, 32767, 32768, 65535)] + [([0, 65535, 1, 32768, 32767, 65535, 0, 0], 8)]
    links = [(0, 0, U // 2, 0, None, 4),
             (1, 1, U, 0, None, 1), (1, 2, U, 0, None, 2), (1, 3, -U // 4, 0, None, 3),
             (2, 0, U // 2, 0, None, 5), (2, 1, U // 2, 0, None, 5, 3),
             (3, 0, U, 0, None, 0), (3, 1, 65535, 1, None, 0, 5)]
    kw = dict(fades=fades, device=DEV, noise_scale_q24=[0, 0, 0, 3 << 20], seed=12, noise_idx_base=1)
    medium = LiveMedium(4, 4, links, **kw)
    silent = LiveMedium(4, 4, [(0, 0, U, 0, None, 0)], **kw)          # row 3 of it: the noise alone
    T = 2051
    host = rng.choice(np.asarray([-32768, 32767, -1, 1, 0, 12345, -20001], np.int16), (4, T))
    host[0, :16] = [-32768, 32767] * 8
    src = torch.from_numpy(host).to(DEV)
    tl = timeline(medium)
    got = medium.mix(src)
    want = expect(tl, medium, host, T)
    same(got, want, "values")
    assert (want[0][host[0] == -32768] == -16384).all() and (want[0][host[0] == 32767] == 16383).all()
    assert want[1].any() and want[2].any()
    noise = expect(timeline(silent), silent, np.zeros_like(host), T)[3]
    assert (want[3] == noise).all() and noise.any()
    same(silent.mix(src)[3], noise, "the noise alone")


# ------------------------------------------------------------------------------------------------------ 3. unity track

LINKS3 = [(0, 0, U, 0, 0), (0, 1, U, 480, 1), (1, 2, 0.5, 512, None), (2, 0, U, 1, 0), (2, 1, -U, 47, 1), (2, 2, U, 48, None),
          (3, 1, 0.25, 9, 0)]


@pytest.mark.parametrize("named", [True, False])
def test_a_unity_track_on_every_link_is_afsk_live_mix_filtered_noise_included(torch_cuda, named):
    """``named`` False: no link names a filter, both entries run their unfiltered paths alone."""
    torch = torch_cuda
    rng = np.random.default_rng(3)
    links = [x if named else x[:4] + (None,) for x in LINKS3]
    kw = dict(device=DEV, noise_scale_q24=[1 << 20, 0, 5 << 20, 1 << 27], seed=7, noise_idx_base=3, max_delay=1024,
              filters=[random_taps(rng, 63), random_taps(rng, 16)])
    filtered = LiveMedium(3, 4, links, **kw)
    faded = LiveMedium(3, 4, [x + (0, 1000003 * i) for i, x in enumerate(links)], fades=[([U] * 4, 8)], **kw)
    assert faded.faded and filtered.filtered and not filtered.faded and filtered.d_fade_knots is None
    assert faded.hist_len == filtered.hist_len == 1024
    tl = timeline(faded)
    for T in (2049, 7, 600):
        host = rng.integers(-32768, 32768, (3, T), dtype=np.int16)
        src = torch.from_numpy(host).to(DEV)
        a, b = filtered.mix(src).clone(), faded.mix(src)
        assert torch.equal(a, b), T
        same(b, expect(tl, faded, host, T), T)
    assert filtered.pos == faded.pos and torch.equal(filtered.d_history, faded.d_history)


# -------------------------------------------------------------------------------------------------------- 4. mixed rows

@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049, 4100])
def test_one_loop_walks_plain_delayed_filtered_faded_and_faded_filtered_links(torch_cuda, T):
    """Three ticks of T, a length per source, noise on two rows.  Row 0 has one link of every kind, in an order that
    puts a faded link in front of and behind every other kind; row 3 has faded filtered links back to back."""
    torch = torch_cuda
    rng = np.random.default_rng(T)
    lens = [T, max(T - 1, 0), T // 2, T + 9, max(T - 8, 0)]
    links = [(0, 0, U // 2), (0, 1, U // 2, 3, None, 0, 11), (0, 2, -U // 2, 5), (0, 3, U // 4, 2, 1, 1, 2 ** 32 - 5),
             (0, 4, U // 2, 40, 0), (0, 0, U // 4, 0, None, 2), (0, 1, U // 4, 7, 0, 0),
             (1, 2, -U, 5, 1), (1, 3, U, 0),
             (2, 4, 0.75, 40, None, 1, 4093), (2, 4, U, 0, 1, -1),
             (3, 3, U // 2, 64, 0, 2, 1), (3, 2, U // 2, 63, 1, 0, 77), (3, 3, U // 4, 0, 0, 1)]
    fades = [(random_knots(rng, 16), 8), (random_knots(rng, 4), 1024), (random_knots(rng, 2), 32768)]
    medium = LiveMedium(5, 4, links, filters=[random_taps(rng, 17), random_taps(rng, 64)], fades=fades, device=DEV,
                        noise_scale_q24=[0, 1 << 20, 5 << 20, 0], seed=21, noise_idx_base=5)
    assert medium.hist_len == 128 and np.diff(medium.row_ptr).tolist() == [7, 2, 2, 3]
    got, want = run(torch, medium, timeline(medium), rng, [T, T, T], lens=lens, tag=(T,))


# ---------------------------------------------------------------------------------------------------- 5. tick sequences

SEQ = (5, 8, 2048, 3000, 13)
LINKS5 = [(0, 0, U, 0, None, 0), (1, 1, U, 300, 0, 0, 17), (2, 0, U // 2, 511, None, 1, 2 ** 31), (2, 1, U // 2, 2, 0, 1)]


@pytest.mark.parametrize("start", [5 * 512 - 3, 7 * 4 * 512 - 5, 2 ** 32 - 100, 3 * 2 ** 32 - 2051],
                         ids=["ring", "track", "2^32", "2^32-in-tick-3"])
def test_tick_sequences_equal_one_tick_of_their_sum(torch_cuda, start):
    """pos starts a few samples before the ring's end (hist_len 512), before the end of the first track (4 knots of 512
    samples: the sequence runs through it twice and more) and before 2^32, where the envelope goes on without a step:
    4 * 512 and 8 * 8 divide 2^32.  The sequence and one mix of the sum both equal the model's, and each other."""
    torch = torch_cuda
    rng = np.random.default_rng(start % 1000)
    fades = [(random_knots(np.random.default_rng(5), 4), 512), (random_knots(np.random.default_rng(6), 8), 8)]
    make = lambda: LiveMedium(2, 3, LINKS5, filters=[random_taps(np.random.default_rng(7), 33)], fades=fades,  # noqa: E731
                              device=DEV, max_delay=512, noise_scale_q24=[0, 1 << 20, 0], seed=5)
    a, b = make(), make()
    assert a.hist_len == 512
    total = sum(SEQ)
    host = rng.integers(-32768, 32768, (2, total), dtype=np.int16)
    src = torch.from_numpy(host).to(DEV)
    a.reset(start)
    b.reset(start)
    whole = a.mix(src)
    same(whole, expect(timeline(a, start), a, host, total), ("whole", start))
    tl, at, parts = timeline(b, start), 0, []
    for T in SEQ:
        got = b.mix(src[:, at: at + T]).clone()
        same(got, expect(tl, b, host[:, at: at + T], T), (start, at, T))
        parts.append(got)
        at += T
    assert torch.equal(torch.cat(parts, dim=1), whole) and a.pos == b.pos == start + total
    assert torch.equal(a.d_history, b.d_history)


def test_state_load_state_and_reset_need_nothing_new(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    fades = [(random_knots(rng, 4), 512), (random_knots(rng, 8), 8)]
    make = lambda: LiveMedium(2, 3, LINKS5, filters=[random_taps(np.random.default_rng(7), 33)], fades=fades,  # noqa: E731
                              device=DEV, max_delay=512)
    host = rng.integers(-20000, 20000, (2, 3000), dtype=np.int16)
    dev = torch.from_numpy(host).to(DEV)
    a = make()
    a.reset(2 ** 32 - 700)
    tl = timeline(a, 2 ** 32 - 700)
    same(a.mix(dev[:, :1001]), expect(tl, a, host[:, :1001], 1001), "before")
    pos, history = a.state()
    assert pos == 2 ** 32 + 301 and history.shape == (2, 512) and (history == host[:, 1001 - 512: 1001]).all()
    b = make()
    b.load_state(pos, history)
    got_a, got_b = a.mix(dev[:, 1001:]), b.mix(dev[:, 1001:])
    assert torch.equal(got_a, got_b)
    same(got_b, expect(tl, a, host[:, 1001:], 1999), "after load_state")
    b.reset()
    fresh = make()
    assert torch.equal(b.mix(dev[:, :2000]), fresh.mix(dev[:, :2000]))


# -------------------------------------------------------------------------------------------------- 6. rewriting knots

def test_knots_rewritten_between_two_mixes_count_in_the_second(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    first, second = random_knots(rng, 8), random_knots(rng, 8)
    links = [(0, 0, U, 0, None, 0), (1, 1, U, 5, 0, 0, 100), (2, 0, U // 2, 0, None, 1)]
    medium = LiveMedium(2, 3, links, filters=[random_taps(rng, 9)], fades=[(first, 64), ([U, U // 2], 8)], device=DEV)
    tl = timeline(medium)
    T = 1500
    host = rng.integers(-32768, 32768, (2, T), dtype=np.int16)
    src = torch.from_numpy(host).to(DEV)
    one = medium.mix(src).clone()
    same(one, expect(tl, medium, host, T), "first knots")
    medium.d_fade_knots[:8] = torch.from_numpy(np.asarray(second, np.uint16)).to(DEV)            # in place: the address stays
    assert medium.d_fade_knots.cpu().numpy().tolist() == second + [U, U // 2]
    two = medium.mix(src).clone()
    want = expect(tl, medium, host, T)                              # (reads the knots off the device)
    same(two, want, "second knots")
    # the second mix is not the first knots' second mix
    stale = FD.Timeline(2, medium.hist_len)
    t = dict(tables_of(medium), fade_knots=np.asarray(first + [U, U // 2], np.uint16))
    for _ in range(2):
        old = stale.mix(host, n_out=3, T=T, **t)
    assert (old[:2] != want[:2]).any() and (old[2] == want[2]).all()


# ----------------------------------------------------------------------------------------------------- 7. graph capture

def test_a_captured_mix_replays_over_ticks_like_eager(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    T, ticks = 2048, 4
    links = [(0, 0, U, 0, 0, 0), (0, 1, U // 2, 480, 1, 1, 9), (1, 2, 0.5, 100, None, 0, 12345), (2, 0, U, 1),
             (2, 1, -U, 2047, 1), (3, 1, 0.25, 9, 0, 1)]
    fades = [(random_knots(rng, 16), 256), (random_knots(rng, 2), 2048)]
    filters = [live.fir_design(63, 0, 3000), live.fir_design(255, 300, 3000)]
    make = lambda: LiveMedium(3, 4, links, filters=filters, fades=fades, device=DEV,  # noqa: E731
                              noise_scale_q24=[1 << 20, 0, 5 << 20, 0], seed=9, max_delay=4096)
    host = rng.integers(-20000, 20000, (3, ticks * T), dtype=np.int16)
    dev = torch.from_numpy(host).to(DEV)
    eager, want = make(), []
    tl = timeline(eager)
    for t in range(ticks):
        got = eager.mix(dev[:, t * T:(t + 1) * T])
        want.append(expect(tl, eager, host[:, t * T:(t + 1) * T], T))
        same(got, want[-1], ("eager", t))
    medium = make()
    src = torch.zeros((3, T), dtype=torch.int16, device=DEV)
    out = torch.zeros((4, T), dtype=torch.int16, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):              # one linear chain of three kernels
            medium.mix(src, out=out, stream=side)
    torch.cuda.synchronize()
    medium.reset()                                              # (the capture ran nothing)
    torch.cuda.synchronize()
    for t in range(ticks):
        src.copy_(dev[:, t * T:(t + 1) * T])
        graph.replay()
        same(out, want[t], ("replay", t))
    assert medium.pos == ticks * T and torch.equal(medium.d_history, eager.d_history)
    torch.cuda.synchronize()
    del graph


# ------------------------------------------------------------------------------------------- 8. broken device tables

def test_fade_tables_out_of_range_on_the_device_are_clamped_and_ignored(torch_cuda):
    """The tables are overwritten where they lie, behind the check: a track index outside the table and a track without
    knots are silent, fade_ptr is clamped into the knots, a knot count that is no power of two is rounded down, the shift
    is clamped to 3 ... 15.  The knots lie between two runs of 65535 that no clamped index reaches: the expected rows are
    the model's with the same clamps over the knots alone, so a knot read from outside them would show."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    T = 700
    fades = [(random_knots(rng, 16), 8), (random_knots(rng, 8), 16), (random_knots(rng, 4), 64)]           # 28 knots
    links = [(0, 0, U, 0, None, 0), (1, 1, U, 3, 0, 1, 5), (2, 0, U, 1, None, 2), (2, 1, U // 2, 0, 0, 1), (3, 1, U, 2, None, 2, 9),
             (3, 0, U // 2, 5)]
    medium = LiveMedium(2, 4, links, filters=[random_taps(rng, 20)], fades=fades, device=DEV)
    n = medium.fade_knots.size
    guard = torch.from_numpy(np.full(n + 64, 65535, np.uint16)).to(DEV)
    guard[32:32 + n] = medium.d_fade_knots
    medium.d_fade_knots = guard[32:32 + n]                          # the knots between two runs of 65535
    tl = timeline(medium)
    edits = [
        dict(),
        dict(link_fade=[-2, 3, 2 ** 31 - 1, 1, -2 ** 31, -1]),                    # outside the table: silent
        dict(link_fade=[0, 1, 2, 1, 2, -1], fade_shift=[2, 16, -2 ** 31]),         # clamped to 3, 15, 3
        dict(fade_shift=[2 ** 31 - 1, 0, 15], fade_ptr=[0, 7, 10, 28]),            # L: 7 -> 4, 3 -> 2, 18 -> 16
        dict(fade_ptr=[-5, 2 ** 31 - 1, 100, 50]),                                 # clamped: 28 -> 16 knots, 0, 0
        dict(fade_ptr=[27, 40, -2 ** 31, 29]),                                     # 1 knot (the last); 0; 28 -> 16
        dict(fade_ptr=[28, 28, 12, 13], fade_shift=[3, 4, 5]),                     # none, none, 1
    ]
    for tick, edit in enumerate(edits):
        for name, values in edit.items():
            getattr(medium, "d_" + name).copy_(torch.tensor(values, dtype=torch.int32))
        host = rng.integers(-32768, 32768, (2, T + 3), dtype=np.int16)
        src, _ = strided(torch, 2, T, 1)
        upload(torch, host, src)
        out, flat = strided(torch, 4, T, 3, fill=POISON)
        got = medium.mix(src, T, out=out)
        want = expect(tl, medium, host, T)
        same(got, want, tick)
        rest = torch.ones_like(flat, dtype=torch.bool)
        rest.as_strided((4, T), (T + 3, 1), 3).fill_(False)
        assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
        if tick == 1:
            assert not want[0].any() and not want[1].any() and want[2].any() and want[3].any()
        if tick == 4:
            assert want[0].any() and not want[1].any()
        if tick == 6:
            assert not want[0].any() and not want[1].any() and want[2].any()
    around = guard.cpu().numpy()
    assert (around[:32] == 65535).all() and (around[32 + n:] == 65535).all()


# ------------------------------------------------------------------------------------------------------ 9. the loop

PAYLOADS = (b"Hello World! 0123456789", b"the second one sinks 42")
LOOP_T = 4096
LOOP_P = 12                                                         # 4096 samples per knot
LOOP_L = 64


def loop_track(start1, n1, start2, n2, total):
    """Unity over the first message, 0.25 over the second, the one-period ramp between them inside the idle gap; the
    track's wrap back to unity lies behind the run."""
    per = 1 << LOOP_P
    ramp = -(-(start1 + n1) // per)                                 # the first knot at or behind the first message's end
    assert start1 + n1 <= ramp * per and (ramp + 1) * per <= start2, "the ramp does not fit the idle gap"
    assert total <= (LOOP_L - 1) * per, "the run reaches the track's wrap"
    return [U if n <= ramp else U // 4 for n in range(LOOP_L)]


def test_a_link_that_sinks_to_a_quarter_carries_the_first_message_and_hides_the_second(torch_cuda):
    """A 1200-baud transmitter channel (training 0.5 s) over one faded link into a streaming receiver with default
    thresholds.  The second message is submitted after the first has ended and two knot periods of idle pulls have
    passed; the track is built from the starts ``submit`` returned.  What the receiver reports is what the oracle's
    gate and decoder report on the MODEL's rows, and on that list -- not on the device's answer -- the first payload
    decodes and the second, a quarter of the amplitude and under the gate's 18000, opens no burst."""
    torch = torch_cuda
    tx = LiveTransmitter(1, 1200, 0.5, queue_depth=2, max_payload_len=32, device=DEV)
    rx = LiveReceiver(1, [40], max_burst_len=None, max_payload_len=32, max_chunk_len=LOOP_T, device=DEV)
    msg = int(tx.message_len(len(PAYLOADS[0]), channels=[0])[0])
    assert msg == int(tx.message_len(len(PAYLOADS[1]), channels=[0])[0])
    first_ticks = -(-msg // LOOP_T) + 3                             # the message, then at least two periods of idle pulls
    ticks = 2 * first_ticks
    pulled = torch.zeros((ticks, 1, LOOP_T), dtype=torch.int16, device=DEV)
    status, start, n = tx.submit([0], [PAYLOADS[0]]).cpu()
    assert status[0] == _native.LIVE_TX_QUEUED
    spans = [(int(start[0]), int(n[0]))]
    for t in range(first_ticks):
        tx.pull(LOOP_T, out=pulled[t])
    status, start, n = tx.submit([0], [PAYLOADS[1]]).cpu()
    assert status[0] == _native.LIVE_TX_QUEUED
    spans.append((int(start[0]), int(n[0])))
    for t in range(first_ticks, ticks):
        tx.pull(LOOP_T, out=pulled[t])
    torch.cuda.synchronize()
    assert not bool(tx.pending.any())
    (s1, n1), (s2, n2) = spans
    assert s2 >= s1 + n1 + 2 * (1 << LOOP_P)
    knots = loop_track(s1, n1, s2, n2, ticks * LOOP_T)
    medium = LiveMedium(1, 1, [(0, 0, U, 0, None, 0)], fades=[(knots, 1 << LOOP_P)], device=DEV)
    chunk = torch.zeros((1, LOOP_T), dtype=torch.int16, device=DEV)
    tl, rows, heard = timeline(medium), [], [[]]
    out = rx.alloc_result()
    sent = pulled.cpu().numpy()
    for t in range(ticks):
        medium.mix(pulled[t], out=chunk)
        rows.append(expect(tl, medium, sent[t], LOOP_T))
        same(chunk, rows[-1], ("loop", t))
        collect(rx.push(chunk, out=out), heard)
    collect(rx.flush(out=out), heard)
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    rows = np.concatenate(rows, axis=1)[0]
    sent = np.concatenate(list(sent), axis=1)[0]
    assert (rows[s1: s1 + n1] == sent[s1: s1 + n1]).all() and np.abs(sent[s1: s1 + n1].astype(int)).max() >= 18000
    quiet = np.abs(rows[s2: s2 + n2].astype(int))
    assert 0 < quiet.max() < 18000 and (rows[s2: s2 + n2] == sent[s2: s2 + n2].astype(int) >> 2).all()
    want = expected(rows, 40, 18000, 14000, 32)
    assert same_bursts(heard[0], want), (heard[0], want)
    assert [w["bytes"] for w in want] == [PAYLOADS[0]] and want[0]["status"] == _native.ST_OK
    assert want[0]["start"] + want[0]["len"] <= s2                    # the one burst is the first message's
