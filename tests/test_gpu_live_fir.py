"""GPU parity (-m gpu) of the filtered live medium: ``LiveMedium(filters=)`` (afsk_live_mix_filtered:
live_mix_fir_kernel, live_mix_history_kernel, live_mix_advance_kernel) against the numpy model over an explicit timeline
(tests/live_fir_model.py), sample for sample.

Expected values never come from the code under test: the mix is the model's (one whole signal per source, no ring, the
rule summed in int64), its noise the CPU oracle's generator.  Two tests hold the device against itself where the header
says two things are equal (the identity filter against afsk_live_mix_delayed, a captured graph against eager), and both
sides against the model.  The last test holds the medium against existing pieces: a LiveTransmitter's tones through a
3 kHz and a 6 kHz low-pass into a streaming LiveReceiver, whose bursts must be what the oracle's gate and decoder report
on the MODEL's rows.  Integer samples: every comparison is exact.  Shapes stay small (n_src <= 6, n_out <= 4, T <= 4200
per mix, one check mix of a sum above that): K, T, the ring and the lengths sit at the edges of the kernel's paths --
the 16-tap chunk, the 8 columns of a thread, the 2048-column tile, the ring's end."""
import numpy as np
import pytest

from afskmodem_amd import _native, live
from afskmodem_amd.live import LiveMedium, LiveReceiver, LiveTransmitter
from tests import live_fir_model as F
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
    """The link and filter tables as they lie ON THE DEVICE now."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    return dict(row_ptr=host(medium.d_row_ptr), link_src=host(medium.d_link_src), link_gain_q15=host(medium.d_link_gain_q15),
                link_delay=host(medium.d_link_delay), link_filter=host(medium.d_link_filter),
                filter_ptr=host(medium.d_filter_ptr), filter_taps=host(medium.d_filter_taps))


def expect(tl, medium, src, T, lens=None):
    """The model's next mix over the device's tables; ``tl``: the ``F.Timeline`` that follows ``medium``."""
    scale = None if medium.d_noise_scale_q24 is None else medium.d_noise_scale_q24.cpu().numpy()
    return tl.mix(src, n_out=medium.n_out, T=T, src_lens=lens, noise_scale_q24=scale, seed=medium.seed,
                  noise_idx_base=medium.noise_idx_base, **tables_of(medium))


def timeline(medium, pos=0):
    return F.Timeline(medium.n_src, medium.hist_len, pos)


def random_taps(rng, K):
    """K taps whose magnitudes sum to at most 65535, the first and the last not 0."""
    top = min(32767, 65535 // K)
    h = rng.integers(-top, top + 1, K)
    h[0], h[-1] = top, -top
    return [int(t) for t in h]


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


# ----------------------------------------------------------------------------------------------------- 1. K and reach

@pytest.mark.parametrize("K", [1, 2, 3, 15, 16, 17, 255, 256])
def test_every_chunk_edge_of_k_at_both_delay_parities_and_a_reach_of_hist_len(torch_cuda, K):
    torch = torch_cuda
    rng = np.random.default_rng(K)
    H = live.medium_hist_len(K + 1)
    last = H - (K - 1)                                              # the delay at which the reach is exactly hist_len
    links = [(0, 0, U, 0, 0), (1, 1, U, 1, 0), (2, 0, -U // 2, last, 0), (3, 1, U, max(last - 1, 0), 0)]
    medium = LiveMedium(2, 4, links, filters=[random_taps(rng, K)], device=DEV)
    assert medium.filtered and medium.delayed and medium.hist_len == H and medium.max_delay == last + K - 1 == H
    assert medium.n_filters == 1 and medium.filter_ptr.tolist() == [0, K] and medium.filter_taps.dtype == np.int16
    tl = timeline(medium)
    got, want = run(torch, medium, tl, rng, [H + 5, 2049, 37], tag=(K,))
    assert all(want[r].any() for r in range(4))


# ------------------------------------------------------------------------------------------- 2. T around 8 and the tile

@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049, 4100])
def test_every_tail_of_t_where_threads_beyond_t_still_stage(torch_cuda, T):
    """Three ticks of T, a length per source, noise on two rows: in the last tile the threads beyond column T have no
    column of their own and stage the window all the same."""
    torch = torch_cuda
    rng = np.random.default_rng(T)
    lens = [T, max(T - 1, 0), T // 2, T + 9, max(T - 8, 0)]
    links = [(0, 0, U, 0, 0), (0, 1, U // 2, 3, 1), (1, 2, -U, 5, 1), (1, 3, U, 0), (2, 4, 0.75, 40, 0), (2, 4, U, 0, 1),
             (3, 3, U, 64, None)]
    medium = LiveMedium(5, 4, links, filters=[random_taps(rng, 17), random_taps(rng, 64)], device=DEV,
                        noise_scale_q24=[0, 1 << 20, 5 << 20, 0], seed=21, noise_idx_base=5)
    assert medium.hist_len == 128
    run(torch, medium, timeline(medium), rng, [T, T, T], lens=lens, tag=(T,))


# -------------------------------------------------------------------------------------------------- 3. the ring's end

SEQ = (5, 8, 2048, 3000, 13)


@pytest.mark.parametrize("hist_len,K,delays,back", [(8, 8, (0, 1), 3), (8, 3, (5, 6), 1), (8, 1, (8, 7), 7),
                                                   (512, 256, (257, 0), 100), (512, 256, (256, 1), 7)])
def test_tick_sequences_across_the_rings_end_equal_one_tick_of_their_sum(torch_cuda, hist_len, K, delays, back):
    """pos starts ``back`` samples before the ring's end, so the staged window of the first ticks straddles it; the
    sequence has ticks below, at and above hist_len.  The sequence and one mix of the sum both equal the model's, and
    each other."""
    torch = torch_cuda
    rng = np.random.default_rng(hist_len + K)
    links = [(0, 0, U, delays[0], 0), (1, 1, U, delays[1], 0), (2, 0, U // 2, delays[1], 0), (2, 1, U // 2, 2)]
    make = lambda: LiveMedium(2, 3, links, filters=[random_taps(np.random.default_rng(K), K)], device=DEV,  # noqa: E731
                              max_delay=hist_len)
    a, b = make(), make()
    assert a.hist_len == hist_len
    start = 5 * hist_len - back
    total = sum(SEQ)
    host = rng.integers(-32768, 32768, (2, total), dtype=np.int16)
    src = torch.from_numpy(host).to(DEV)
    a.reset(start)
    b.reset(start)
    whole = a.mix(src)
    same(whole, expect(timeline(a, start), a, host, total), ("whole", hist_len, K))
    tl, at, parts = timeline(b, start), 0, []
    for T in SEQ:
        got = b.mix(src[:, at: at + T]).clone()
        same(got, expect(tl, b, host[:, at: at + T], T), (hist_len, K, at, T))
        parts.append(got)
        at += T
    assert torch.equal(torch.cat(parts, dim=1), whole) and a.pos == b.pos == start + total
    assert torch.equal(a.d_history, b.d_history)


# ---------------------------------------------------------------------------------------------------------- 4. lengths

@pytest.mark.parametrize("T", [19, 2049])
def test_a_length_inside_the_window_and_stale_columns_behind_it(torch_cuda, T):
    """Every source holds a marker from its length on; the filter's window reaches across the length, into the marker's
    columns, and must read zeros there.  |signal| <= 9000 and sum |h| <= 23062 bound every output by 9000 * 23062 / 16384
    < 12669: the marker, 32767, through any tap would show."""
    torch = torch_cuda
    rng = np.random.default_rng(T)
    lp = live.fir_design(63, 0, 3000)
    links = [(0, s, U, 0, 0) for s in range(3)] + [(1, s, U, 7, 0) for s in range(3, 6)] + \
        [(2, 2, U, T // 2, 0), (2, 5, -U, 1, 0), (3, 4, U, 0, 0), (3, 4, U // 2, 33)]
    medium = LiveMedium(6, 4, links, filters=[lp], device=DEV, max_delay=4096)
    tl = timeline(medium)
    for tick, given in enumerate(([-5, 0, 1, 5, T, T + 9], None, [T, T - 1, T // 2, 2, 0, T - 8], [0] * 6)):
        host = rng.integers(-9000, 9001, (6, T), dtype=np.int16)
        for s, ln in enumerate(given or [T] * 6):
            host[s, max(min(ln, T), 0):] = POISON
        d_lens = None if given is None else torch.tensor(given, dtype=torch.int32, device=DEV)
        got = medium.mix(torch.from_numpy(host).to(DEV), lengths=d_lens)
        want = expect(tl, medium, host, T, given)
        same(got, want, (T, tick))
        assert np.abs(want.astype(int)).max() < 12669 * 2                     # (rows 0 and 1 sum three sources: clip)
    assert want.any()                                               # all lengths 0: the filters still ring out


# ------------------------------------------------------------------------------------------- 5. saturation and floor

def test_the_filter_sum_saturates_at_both_ends_and_floors(torch_cuda):
    torch = torch_cuda
    neg2, neg256 = [-32768, -32767], [-256] * 255 + [-255]           # sum |h| = 65535 twice
    assert sum(-t for t in neg2) == sum(-t for t in neg256) == 65535
    filters = [neg2, neg256, [32767, 32767], [Q14 // 2], [-1]]
    links = [(0, 0, U, 0, 0), (1, 0, U, 0, 1), (2, 1, U, 0, 0), (3, 0, U, 0, 2),
             (0, 2, U, 0, 3), (1, 2, U, 0, 4), (2, 2, -U, 0, 3)]     # (source 2 is silent in the first mix)
    medium = LiveMedium(3, 4, links, filters=filters, device=DEV)
    T = 600
    host = np.zeros((3, T), np.int16)
    host[0], host[1] = -32768, 32767
    tl = timeline(medium)
    got = medium.mix(torch.from_numpy(host).to(DEV))
    want = expect(tl, medium, host, T)
    same(got, want, "saturation")
    # v = 65535 * 32768 = 2147450880 from column K - 1 on: >> 14 = 131070, clamped to 32767 (one tap of -256: 512)
    assert (want[0] == 32767).all() and (want[1, 255:] == 32767).all() and want[1, :2].tolist() == [512, 1024]
    assert (want[2, 1:] == -32768).all() and (want[3, 1:] == -32768).all()   # the mirror: 65535 * -32767, 65534 * -32768
    host[:2] = 0
    host[2] = np.arange(T) - 300                                                # odd negative samples: >> floors
    got = medium.mix(torch.from_numpy(host).to(DEV))
    want = expect(tl, medium, host, T)
    same(got, want, "floor")
    x = host[2, 256:].astype(np.int64)
    assert (want[0, 256:] == x >> 1).all() and (want[1, 256:] == (-x) >> 14).all() and (want[2, 256:] == -(x >> 1)).all()
    assert want[0, 299] == -1 and want[1, 301] == -1 and want[2, 297] == 2      # -1 / 2 -> -1, -1 / 16384 -> -1, -(-3 >> 1)


# -------------------------------------------------------------------------------------------------------- 6. mixed rows

def test_one_row_hears_filtered_and_unfiltered_links_echoes_zero_gains_and_negative_gains(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    filters = [live.fir_design(63, 0, 3000), live.fir_design(31, 300, 6000), [0.5, 0, 0, -0.25], [Q14]]
    links = [(0, 0, U, 3, 0), (0, 1, U // 2, 9), (0, 0, -U // 2, 0, 1), (0, 0, U // 4, 40, 2), (0, 2, 0, 0, 0),
             (0, 2, -65535, 1, 3), (0, 1, -U, 0, None), (0, 1, U // 3, 17, 2), (0, 0, 0, 5),
             (1, 2, U, 0), (1, 2, U, 1),                                     # a row without a filtered link
             (3, 1, -U, 100, 0), (3, 1, -U, 101, 0), (3, 1, 65535, 0, 1)]   # filtered links only, back to back
    medium = LiveMedium(3, 4, links, filters=filters, device=DEV, noise_scale_q24=[1 << 20, 0, 3 << 20, 0], seed=4)
    assert np.diff(medium.row_ptr).tolist() == [9, 2, 0, 3] and medium.hist_len == 256
    tl = timeline(medium)
    got, want = run(torch, medium, tl, rng, [100, 2049, 8, 4100], full=12000)
    assert want[0].any() and want[1].any() and want[3].any()


# ---------------------------------------------------------------------------------------------- 7. the two identities

def test_the_identity_filter_on_every_link_is_afsk_live_mix_delayed_noise_included(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    links = [(0, 0, U, 0), (0, 1, U, 480), (1, 2, 0.5, 512), (2, 0, U, 1), (2, 1, -U, 47), (2, 2, U, 48), (3, 1, 0.25, 9)]
    kw = dict(device=DEV, noise_scale_q24=[1 << 20, 0, 5 << 20, 1 << 27], seed=7, noise_idx_base=3, max_delay=512)
    delayed = LiveMedium(3, 4, links, **kw)
    filtered = LiveMedium(3, 4, [x + (0,) for x in links], filters=[[1.0]], **kw)
    assert filtered.filtered and not delayed.filtered and delayed.d_filter_taps is None and delayed.n_filters == 0
    assert filtered.hist_len == delayed.hist_len == 512
    tl = timeline(filtered)
    for T in (2049, 7, 600):
        host = rng.integers(-30000, 30000, (3, T), dtype=np.int16)
        src = torch.from_numpy(host).to(DEV)
        a, b = delayed.mix(src).clone(), filtered.mix(src)
        assert torch.equal(a, b), T
        same(b, expect(tl, filtered, host, T), T)
    assert delayed.pos == filtered.pos and torch.equal(delayed.d_history, filtered.d_history)


@pytest.mark.parametrize("n,d", [(1, 0), (5, 3), (16, 1), (255, 1)])
def test_zero_taps_in_front_of_unity_are_that_much_more_delay(torch_cuda, n, d):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    a = LiveMedium(1, 1, [(0, 0, 12345, d, 0)], filters=[[0] * n + [Q14]], device=DEV, max_delay=256)
    b = LiveMedium(1, 1, [(0, 0, 12345, d + n)], device=DEV, max_delay=256)
    tl = timeline(a)
    for T in (300, 1, 2049):
        host = rng.integers(-32768, 32768, (1, T), dtype=np.int16)
        src = torch.from_numpy(host).to(DEV)
        got = a.mix(src)
        assert torch.equal(got, b.mix(src)), (n, d, T)
        same(got, expect(tl, a, host, T), (n, d, T))


# ------------------------------------------------------------------------------------------- 8. broken device tables

def test_filter_tables_out_of_range_on_the_device_are_clamped_and_ignored(torch_cuda):
    """The tables are overwritten where they lie, behind the check: a filter index outside the table and K = 0 are
    silent, filter_ptr is clamped into the taps, K = 300 counts as 256.  The expected rows are the model's with the same
    clamps; the poison around ``out`` and around the history stays."""
    torch = torch_cuda
    rng = np.random.default_rng(8)
    T, H = 700, 512
    filters = [random_taps(rng, 256), random_taps(rng, 100), [Q14 // 2, Q14 // 4]]            # 358 taps
    links = [(0, 0, U, 0, 0), (1, 1, U, 3, 1), (2, 0, U, 1, 2), (2, 1, U // 2, 0, 1), (3, 1, U, 2, 2), (3, 0, U // 2, 5)]
    medium = LiveMedium(2, 4, links, filters=filters, device=DEV, max_delay=H)
    guard = torch.full((4, H), POISON, dtype=torch.int16, device=DEV)
    guard[1:3].zero_()
    medium.d_history = guard[1:3]                                   # the history between two rows of poison
    tl = timeline(medium)
    edits = [
        dict(),
        dict(link_filter=[-2, 3, 2 ** 31 - 1, 1, -2 ** 31, -1]),                  # outside the table: silent
        dict(link_filter=[0, 1, 2, 1, 2, -1], filter_ptr=[0, 300, 300, 358]),      # K = 300 -> 256; K = 0: silent
        dict(filter_ptr=[-5, 2 ** 31 - 1, 100, 50]),                               # clamped: K = 256 (of 358), 0, 0
        dict(filter_ptr=[357, 358, -2 ** 31, 400]),                                # K = 1, 0, 358 - 0 -> 256
        dict(filter_ptr=[0, 256, 356, 358], link_delay=[2 ** 31 - 1, -7, 511, 500, 600, 513]),  # delays against the reach
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
        assert bool((guard[0] == POISON).all()) and bool((guard[3] == POISON).all()), "the history's neighbours were written"
        if tick == 1:
            assert not want[0].any() and not want[1].any() and want[2].any() and want[3].any()
        if tick == 2:
            assert want[0].any() and not want[1].any()


# ------------------------------------------------------------------------------------------- 9. capture and restart

LINKS9 = [(0, 0, U, 0, 0), (0, 1, U // 2, 480, 1), (1, 2, 0.5, 100, 0), (2, 0, U, 1), (2, 1, -U, 2047, 1), (3, 1, 0.25, 9, 0)]


def medium9(**kw):
    return LiveMedium(3, 4, LINKS9, filters=[live.fir_design(63, 0, 3000), live.fir_design(255, 300, 3000)], device=DEV,
                      noise_scale_q24=[1 << 20, 0, 5 << 20, 0], seed=9, max_delay=4096, **kw)


def test_a_captured_mix_replays_over_ticks_like_eager(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(9)
    T, ticks = 2048, 5
    host = rng.integers(-20000, 20000, (3, ticks * T), dtype=np.int16)
    dev = torch.from_numpy(host).to(DEV)
    eager, tl, want = medium9(), None, []
    tl = timeline(eager)
    for t in range(ticks):
        got = eager.mix(dev[:, t * T:(t + 1) * T])
        want.append(expect(tl, eager, host[:, t * T:(t + 1) * T], T))
        same(got, want[-1], ("eager", t))
    medium = medium9()
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


def test_state_load_state_and_reset_in_mid_signal(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(10)
    host = rng.integers(-20000, 20000, (3, 9000), dtype=np.int16)
    dev = torch.from_numpy(host).to(DEV)
    a = medium9()
    tl = timeline(a)
    cuts = [0, 3000, 3000 + 4101, 9000]                         # (pos & mask is neither 0 nor a multiple of 8)
    for lo, hi in zip(cuts[:2], cuts[1:3]):
        same(a.mix(dev[:, lo:hi]), expect(tl, a, host[:, lo:hi], hi - lo), (lo, hi))
    pos, history = a.state()
    assert pos == cuts[2] and history.shape == (3, 4096) and (history == host[:, pos - 4096: pos]).all()
    b = medium9()
    b.load_state(pos, history)
    lo, hi = cuts[2], cuts[3]
    got_a, got_b = a.mix(dev[:, lo:hi]), b.mix(dev[:, lo:hi])
    assert torch.equal(got_a, got_b)
    same(got_b, expect(tl, a, host[:, lo:hi], hi - lo), "after load_state")
    fresh = medium9()
    first = fresh.mix(dev[:, :2000]).clone()
    b.reset()
    assert b.pos == 0 and not bool(b.d_history.any())
    assert torch.equal(b.mix(dev[:, :2000]), first)             # what was sent before the reset is forgotten
    same(first, expect(timeline(fresh), fresh, host[:, :2000], 2000), "a new medium")


# --------------------------------------------------------------------------------------------- 10. which rates survive

PAYLOAD = b"Hello World! 0123456789"
E2E_T = 4096


@pytest.mark.parametrize("spec,survives", [((63, 0, 3000), False), ((31, 0, 6000), True)])
def test_a_3_khz_link_carries_1200_baud_and_silences_2400_baud_and_6_khz_carries_both(torch_cuda, spec, survives):
    """A two-channel transmitter at 1200 and 2400 baud (training 0.5 s), every channel over its own link through one
    low-pass, into a streaming receiver with default thresholds.  What the receiver reports is what the oracle's gate
    and decoder report on the MODEL's rows; and, as the unmodified reference decoder showed, the 1200-baud channel
    returns the payload under both filters, the 2400-baud channel under the 6 kHz one only -- under 3 kHz its tones,
    square waves that keep most of their shape in harmonics, never open the gate: no burst at all."""
    torch = torch_cuda
    bfs = [40, 20]
    tx = LiveTransmitter(2, [1200, 2400], 0.5, queue_depth=2, max_payload_len=32, device=DEV)
    rx = LiveReceiver(2, bfs, max_burst_len=None, max_payload_len=32, max_chunk_len=E2E_T, device=DEV)
    medium = LiveMedium(2, 2, [(0, 0, U, 0, 0), (1, 1, U, 0, 0)], filters=[live.fir_design(*spec)], device=DEV)
    assert medium.hist_len == {63: 64, 31: 32}[spec[0]] and medium.max_delay == spec[0] - 1   # the reach: taps - 1
    assert (tx.submit([0, 1], [PAYLOAD, PAYLOAD]).cpu()[0] == _native.LIVE_TX_QUEUED).all()
    ticks = -(-int(tx.message_len(len(PAYLOAD), channels=[0])[0]) // E2E_T) + 3
    src = torch.zeros((2, E2E_T), dtype=torch.int16, device=DEV)
    chunk = torch.zeros((2, E2E_T), dtype=torch.int16, device=DEV)
    tl, rows, heard = timeline(medium), [], [[], []]
    out = rx.alloc_result()
    for t in range(ticks):
        tx.pull(E2E_T, out=src)
        medium.mix(src, out=chunk)
        rows.append(expect(tl, medium, src.cpu().numpy(), E2E_T))
        same(chunk, rows[-1], (spec, t))
        collect(rx.push(chunk, out=out), heard)
    collect(rx.flush(out=out), heard)
    torch.cuda.synchronize()
    assert not bool(tx.pending.any())
    rx.close()
    tx.close()
    rows = np.concatenate(rows, axis=1)
    want = [expected(rows[c], bfs[c], 18000, 14000, 32) for c in range(2)]
    for c in range(2):
        assert same_bursts(heard[c], want[c]), (spec, c, heard[c], want[c])
    assert [w["bytes"] for w in want[0]] == [PAYLOAD] and want[0][0]["status"] == _native.ST_OK
    if survives:
        assert [w["bytes"] for w in want[1]] == [PAYLOAD] and want[1][0]["status"] == _native.ST_OK
    else:
        assert want[1] == [] and heard[1] == []
