"""GPU parity (-m gpu) of the delayed live medium: ``LiveMedium`` with delays (afsk_live_mix_delayed:
live_mix_delay_kernel, live_mix_history_kernel, live_mix_advance_kernel) against ``afsk_live_mix`` where every delay is 0
and against the numpy model over an explicit timeline (tests/live_delay_model.py) everywhere else, sample for sample.

Expected values never come from the code under test: the mix is the model's (which keeps every source as one whole
signal and knows no ring), its noise the CPU oracle's generator.  The last tests hold the medium against existing
pieces: the oracle's gate and decoder behind a ``LiveReceiver`` for an echo, the host models of the carrier-sensing
stations (tests/live_tx_hold_model.py) for a carrier that arrives late, and one captured graph of a whole station tick.
Integer samples: every comparison is exact."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, synth
from afskmodem_amd.live import LiveMedium, LiveReceiver, LiveTransmitter, medium_csr, medium_delays
from oracle import afsk_oracle as O
from tests import live_delay_model as D
from tests import live_mix_model as M
from tests import live_tx_hold_model as H
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import collect
from tests.test_gpu_live_mix import same, strided, upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = M.UNITY
POISON = 32767
Q = _native.LIVE_TX_QUEUED


def tables_of(medium):
    """The four link tables as they lie ON THE DEVICE now."""
    return tuple(t.cpu().numpy() for t in (medium.d_row_ptr, medium.d_link_src, medium.d_link_gain_q15,
                                           medium.d_link_delay))


def expect(tl, medium, src, T, lens=None):
    """The model's next mix over the device's tables; ``tl``: the ``D.Timeline`` that follows ``medium``."""
    scale = None if medium.d_noise_scale_q24 is None else medium.d_noise_scale_q24.cpu().numpy()
    return tl.mix(src, *tables_of(medium), medium.n_out, T, src_lens=lens, noise_scale_q24=scale, seed=medium.seed,
                  noise_idx_base=medium.noise_idx_base)


def timeline(medium, pos=0):
    return D.Timeline(medium.n_src, medium.hist_len, pos)


# --------------------------------------------------------------------------- 1. every delay 0: afsk_live_mix's output

@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049])
def test_every_tail_with_every_delay_0_is_afsk_live_mix(torch_cuda, T, noise):
    """Rows at odd sample offsets with stride T + 3, the sources poisoned from their lengths on, ``out`` poisoned outside
    its T columns: two mixes in a row of a delayed medium whose delays are all 0 against the undelayed medium."""
    torch = torch_cuda
    rng = np.random.default_rng(T)
    n_src, n_out = 5, 4
    lens = [T, max(T - 1, 0), T // 2, T + 9, max(T - 8, 0)]
    links = [(1, 3, U), (2, 0, U // 2), (2, 1, -U // 2), (3, 0, U), (3, 1, U), (3, 2, 0.75), (3, 4, -U), (3, 1, U)]
    kw = dict(noise_scale_q24=[1 << 20, 5 << 20, 0, 1 << 24], seed=21, noise_idx_base=5) if noise else {}
    plain = LiveMedium(n_src, n_out, links, device=DEV, **kw)
    delayed = LiveMedium(n_src, n_out, [x + (0,) for x in links], device=DEV, max_delay=8, **kw)
    assert delayed.delayed and delayed.hist_len == 8 and not plain.delayed and plain.d_history is None
    src, _ = strided(torch, n_src, T, 1)
    for tick in range(2):
        host = rng.integers(-32768, 32768, (n_src, T + 3), dtype=np.int16)
        for s in range(n_src):
            host[s, max(min(lens[s], T), 0):] = POISON
        upload(torch, host, src)
        want = plain.mix(src, T, lengths=lens).clone()
        out, flat = strided(torch, n_out, T, 3, fill=POISON)
        got = delayed.mix(src, T, out=out, lengths=lens)
        assert tuple(got.shape) == (n_out, T) and got.data_ptr() == out.data_ptr()
        assert torch.equal(got, want), (T, tick)
        rest = torch.ones_like(flat, dtype=torch.bool)
        rest.as_strided((n_out, T), (T + 3, 1), 3).fill_(False)
        assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
    assert delayed.pos == 2 * T and bool(want[1:].any())
    if noise:
        assert plain.pos == 2 * T


# ------------------------------------------------------------------------------------------ 2. delays against the model

def delay_links(n_src, hist_len, Ts):
    """One unity row per delay of the issue's list, then rows of degree 0, 2 (the same source twice, at two delays) and
    5 (two sources twice)."""
    ds = sorted({d for d in [0, 1, 7, 8, 9, hist_len - 1, hist_len] + [T + e for T in Ts for e in (-1, 0, 1)]
                 if 0 <= d <= hist_len})
    links = [(i, i % n_src, U, d) for i, d in enumerate(ds)]
    r = len(ds) + 1                                                  # row len(ds): no links
    links += [(r, 1, U, 0), (r, 1, U // 2, min(10, hist_len))]
    links += [(r + 1, 0, -U, hist_len), (r + 1, 2, 65535, 1), (r + 1, 0, U // 4, 3), (r + 1, 1, U, hist_len - 1),
              (r + 1, 2, -U // 2, 7)]
    return r + 2, links


@pytest.mark.parametrize("hist_len,Ts", [(8, [5, 8, 24, 5, 1]), (16, [9, 16, 40, 15]), (4096, [2048, 6000, 2048, 100])])
@pytest.mark.parametrize("noise", [False, True])
def test_delays_over_tick_sequences_below_at_and_above_hist_len(torch_cuda, hist_len, Ts, noise):
    torch = torch_cuda
    rng = np.random.default_rng(hist_len)
    n_src = 3
    n_out, links = delay_links(n_src, hist_len, Ts)
    kw = dict(noise_scale_q24=(np.arange(n_out) % 3) << 20, seed=8, noise_idx_base=2 ** 32 - 3) if noise else {}
    medium = LiveMedium(n_src, n_out, links, device=DEV, max_delay=hist_len, **kw)
    assert medium.hist_len == hist_len and medium.history_bytes == 2 * n_src * hist_len
    degrees = np.diff(medium.row_ptr).tolist()
    assert degrees[-3:] == [0, 2, 5] and set(degrees[:-3]) == {1}
    tl = timeline(medium)
    for i, T in enumerate(Ts):
        host = rng.integers(-32768, 32768, (n_src, T + 3), dtype=np.int16)
        src, _ = strided(torch, n_src, T, 1)
        upload(torch, host, src)
        out, flat = strided(torch, n_out, T, 3, fill=POISON)
        got = medium.mix(src, T, out=out)
        want = expect(tl, medium, host, T)
        same(got, want, (hist_len, i, T))
        rest = torch.ones_like(flat, dtype=torch.bool)
        rest.as_strided((n_out, T), (T + 3, 1), 3).fill_(False)
        assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
        if not noise:
            assert not want[n_out - 3].any()
    assert medium.pos == sum(Ts) == tl.pos


# ------------------------------------------------------------------------------------------------- 3. ring positions

@pytest.mark.parametrize("hist_len,T", [(16, 24), (4096, 2056)])
def test_a_start_1_to_7_samples_before_the_rings_end(torch_cuda, hist_len, T):
    """``pos & (hist_len - 1)`` lies k = 1 ... 7 before the ring's end, so the 8 columns of one thread of the history
    kernel, and later of the mix, cross the wrap."""
    torch = torch_cuda
    rng = np.random.default_rng(3)
    links = [(0, 0, U, 0), (1, 0, U, 1), (2, 1, U, 8), (3, 1, U, hist_len - 3), (4, 0, U, hist_len), (4, 1, U // 2, 5),
             (5, 1, U, 12)]
    medium = LiveMedium(2, 6, links, device=DEV, max_delay=hist_len)
    for k in range(1, 8):
        start = 5 * hist_len - k
        medium.reset(start)
        assert medium.pos == start
        tl = timeline(medium, start)
        for tick in range(3):
            host = rng.integers(-32768, 32768, (2, T), dtype=np.int16)
            got = medium.mix(torch.from_numpy(host).to(DEV))
            same(got, expect(tl, medium, host, T), (hist_len, k, tick))
        assert medium.pos == start + 3 * T


def test_a_position_just_below_2_32_with_noise(torch_cuda):
    """The noise's uint32 sample index and the ring's index both come from the low 32 bits of pos, and both wrap."""
    torch = torch_cuda
    rng = np.random.default_rng(4)
    links = [(0, 0, U, 0), (1, 0, U, 3), (2, 1, U, 16), (3, 1, -U, 9), (3, 0, U // 2, 1)]
    medium = LiveMedium(2, 4, links, device=DEV, max_delay=16, noise_scale_q24=[1 << 20, 0, 5 << 20, 1 << 22], seed=11,
                        noise_idx_base=7)
    start = 2 ** 32 - 5
    medium.reset(start)
    tl = timeline(medium, start)
    for T in (3, 9, 24):
        host = rng.integers(-32768, 32768, (2, T), dtype=np.int16)
        same(medium.mix(torch.from_numpy(host).to(DEV)), expect(tl, medium, host, T), T)
    assert medium.pos == start + 36 > 2 ** 32


# -------------------------------------------------------------------------------------------------- 4. ragged lengths

@pytest.mark.parametrize("T,hist_len", [(19, 32), (2049, 4096)])
def test_columns_beyond_a_length_come_back_as_zeros_through_a_delay(torch_cuda, T, hist_len):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    lens = [-5, 0, 1, 5, T, T + 9]
    links = [(s, s, U, T) for s in range(6)] + [(6 + s, s, U, T - 3) for s in range(6)] + \
        [(12, s, U // 8, hist_len) for s in range(6)] + [(13, 3, U, 0), (13, 3, U, 2)]
    medium = LiveMedium(6, 14, links, device=DEV, max_delay=hist_len)
    tl = timeline(medium)
    hosts = []
    for tick, given in enumerate((lens, None, [T, T, T, 2, 0, -1])):
        host = rng.integers(-9000, 9000, (6, T), dtype=np.int16)
        for s, ln in enumerate(given or [T] * 6):
            host[s, max(min(ln, T), 0):] = POISON                    # the buffer holds poison beyond every length
        hosts.append(host)
        d_lens = None if given is None else torch.tensor(given, dtype=torch.int32, device=DEV)
        got = medium.mix(torch.from_numpy(host).to(DEV), lengths=d_lens)
        want = expect(tl, medium, host, T, given)
        same(got, want, (T, tick))
        if tick == 1:                                                # tick 1 replayed at a delay of exactly T
            assert not want[0].any() and not want[1].any()
            assert want[2, 0] == hosts[0][2, 0] and not want[2, 1:].any()
            assert (want[3, :5] == hosts[0][3, :5]).all() and not want[3, 5:].any()
            assert (want[4] == hosts[0][4]).all() and (want[5] == hosts[0][5]).all()
            assert (np.abs(want[:6].astype(int)) < 9000).all()       # no poison came through


# --------------------------------------------------------------------------------------------------- 5. table clamps

def test_delays_sources_and_row_ptr_out_of_range_on_the_device_are_clamped_and_ignored(torch_cuda):
    """The tables are overwritten where they lie: by construction no index reaches a load unclamped."""
    torch = torch_cuda
    rng = np.random.default_rng(6)
    hist_len, T = 16, 40
    links = [(0, 0, U, 0), (1, 0, U, hist_len), (2, 0, U, 5), (3, 1, U, 5), (4, 1, U, 2), (4, 0, U, 4), (5, 1, U, 0)]
    medium = LiveMedium(2, 6, links, device=DEV, max_delay=hist_len)
    delays = medium.link_delay.copy()
    delays[[2, 3, 5]] = [-3, hist_len + 100, 2 ** 31 - 1]
    medium.d_link_delay.copy_(torch.from_numpy(delays))
    tl = timeline(medium)
    for tick in range(3):
        host = rng.integers(-32768, 32768, (2, T), dtype=np.int16)
        src = torch.from_numpy(host).to(DEV)
        if tick == 1:
            srcs = medium.link_src.copy()
            srcs[[4, 6]] = [2, -1]                                  # outside the matrix: silent, and nothing is read
            medium.d_link_src.copy_(torch.from_numpy(srcs))
        if tick == 2:
            medium.d_row_ptr.copy_(torch.tensor([0, 1, 2, 1, 4, 2 ** 31 - 1, -5], dtype=torch.int32))
            medium.d_link_delay.copy_(torch.tensor([-2 ** 31, 2 ** 31 - 1, -1, 17, 16, 15, 0], dtype=torch.int32))
        want = expect(tl, medium, host, T)
        same(medium.mix(src), want, tick)
        if tick == 0:
            assert (want[2] == want[0]).all() and (want[0] == host[0]).all()      # a delay of -3 is a delay of 0
            assert not want[3, :hist_len].any() and (want[3, hist_len:] == host[1, : T - hist_len]).all()   # + 100: hist_len
        if tick == 1:
            assert not want[5].any() and want[3].any()


# ------------------------------------------------------------------------------------------------- 6. a grid past 65535

def test_70000_source_and_output_rows(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n, T, hist_len = 70000, 8, 8
    r = np.arange(n)
    a, b = r, (r * 7 + 3) % n
    da, db = r % 9, (r // 9) % 9                                     # every delay 0 ... hist_len
    ga, gb = rng.integers(-65535, 65536, n), rng.integers(-65535, 65536, n)
    links = [(i, s, g, d) for i in range(n) for s, g, d in ((int(a[i]), int(ga[i]), int(da[i])),
                                                             (int(b[i]), int(gb[i]), int(db[i])))]
    medium = LiveMedium(n, n, links, device=DEV, max_delay=hist_len)
    assert medium.hist_len == hist_len
    rows = [0, 1, 8, 65535, 65536, 69999]
    srcs = sorted({int(x) for i in rows for x in (a[i], b[i])})
    small = [(k, srcs.index(int(s)), g, d) for k, i in enumerate(rows)
             for s, g, d in ((a[i], int(ga[i]), int(da[i])), (b[i], int(gb[i]), int(db[i])))]
    small_tables = (*medium_csr(len(rows), small), medium_delays(len(rows), small))
    tl = D.Timeline(len(srcs), hist_len)
    X = np.zeros((n, 0), np.int64)
    for tick in range(3):
        host = rng.integers(-32768, 32768, (n, T), dtype=np.int16)
        got = medium.mix(torch.from_numpy(host).to(DEV))
        X = np.concatenate([X, host.astype(np.int64)], axis=1)
        at = X.shape[1] - T + np.arange(T)[None, :]                    # the rule written out over the whole timeline
        xa = np.where(at - da[:, None] >= 0, X[a[:, None], np.maximum(at - da[:, None], 0)], 0)
        xb = np.where(at - db[:, None] >= 0, X[b[:, None], np.maximum(at - db[:, None], 0)], 0)
        want = np.clip(((ga[:, None] * xa) >> 15) + ((gb[:, None] * xb) >> 15), -32768, 32767).astype(np.int16)
        sel = tl.mix(host[srcs], *small_tables, len(rows), T)          # ... held against the model on a few rows
        assert (sel == want[rows]).all(), tick
        same(got, want, ("70000 rows", tick))


# -------------------------------------------------------------------------------------- 7. tick equality, reset, state

NOISE_T = 4096
SCALES = [1 << 20, 0, 5 << 20, 1 << 27]
LINKS7 = [(0, 0, U, 0), (0, 1, U, 480), (1, 2, 0.5, 4096), (2, 0, U, 1), (2, 1, -U, 2047), (2, 2, U, 2048), (3, 1, 0.25, 2049),
          (3, 1, 0.5, 9)]


def noise_case(torch, **kw):
    rng = np.random.default_rng(8)
    host = rng.integers(-30000, 30000, (3, 3 * NOISE_T), dtype=np.int16)
    make = lambda: LiveMedium(3, 4, LINKS7, device=DEV, noise_scale_q24=SCALES, max_delay=4096, **kw)  # noqa: E731
    return host, torch.from_numpy(host).to(DEV), make


def test_two_ticks_of_2048_equal_one_tick_of_4096_and_reset_gives_a_new_medium(torch_cuda):
    torch = torch_cuda
    host, src, make = noise_case(torch, seed=7)
    a, b = make(), make()
    tl = timeline(a)
    for t in range(2):                                               # the second pair reads the first through the ring
        lo = t * NOISE_T
        whole = a.mix(src[:, lo: lo + NOISE_T])
        halves = torch.cat([b.mix(src[:, lo: lo + 2048]).clone(), b.mix(src[:, lo + 2048: lo + NOISE_T]).clone()], dim=1)
        assert torch.equal(whole, halves), t
        same(whole, expect(tl, a, host[:, lo: lo + NOISE_T], NOISE_T), ("4096 at once", t))
    assert a.pos == b.pos == 2 * NOISE_T
    fresh = make()
    first = fresh.mix(src[:, :NOISE_T]).clone()
    b.reset()
    assert b.pos == 0 and not bool(b.d_history.any())
    assert torch.equal(b.mix(src[:, :NOISE_T]), first)                # what was sent before the reset is forgotten
    same(first, expect(timeline(fresh), fresh, host[:, :NOISE_T], NOISE_T), "a new medium")


def test_state_and_load_state_continue_bit_for_bit(torch_cuda):
    torch = torch_cuda
    host, src, make = noise_case(torch, seed=9, noise_idx_base=40)
    a = make()
    tl = timeline(a)
    cuts = [0, 3000, 3000 + 4101, 3 * NOISE_T]                      # (pos & mask is neither 0 nor a multiple of 8)
    for lo, hi in zip(cuts[:2], cuts[1:3]):
        same(a.mix(src[:, lo:hi]), expect(tl, a, host[:, lo:hi], hi - lo), (lo, hi))
    pos, history = a.state()
    assert pos == cuts[2] and history.shape == (3, 4096) and history.dtype == np.int16
    assert (history == host[:, pos - 4096: pos]).all()                # time order, oldest first
    b = make()
    b.load_state(pos, history)
    assert b.pos == pos and torch.equal(b.d_history, a.d_history)
    lo, hi = cuts[2], cuts[3]
    got_a, got_b = a.mix(src[:, lo:hi]), b.mix(src[:, lo:hi])
    assert torch.equal(got_a, got_b)
    same(got_b, expect(tl, a, host[:, lo:hi], hi - lo), "after load_state")
    early = make()
    early.mix(src[:, :100])
    p, h = early.state()                                             # less sent than the history holds: zeros in front
    assert p == 100 and not h[:, :-100].any() and (h[:, -100:] == host[:, :100]).all()
    plain = LiveMedium(3, 4, [x[:3] for x in LINKS7], device=DEV)
    assert plain.state()[0] == 0 and plain.state()[1].shape == (3, 0)
    with pytest.raises(ValueError):
        b.load_state(0, history[:, :8])


# ---------------------------------------------------------------------------------------------------------- 8. an echo

def test_an_echo_a_quarter_symbol_late_decodes_to_what_the_oracle_decodes(torch_cuda):
    """One 1200-baud burst over a unity link and a second link of the same source at half the level, 10 samples (a
    quarter symbol) late.  The oracle's gate and decoder on the MODEL's row say what the receiver must report; the same
    listener without the echo reports the payload."""
    torch = torch_cuda
    T = 2048
    payload = b"multipath"
    wav = afskmodem.Transmitter(1200, 0.1).wav_samples(payload)
    total = -(-(T + 100 + wav.size + 3 * T) // T) * T
    host = np.zeros((1, total), np.int16)
    host[0, T + 100: T + 100 + wav.size] = wav
    src = torch.from_numpy(host).to(DEV)
    rows = {}
    for echo in (False, True):
        links = [(0, 0, U, 0)] + ([(0, 0, 0.5, 10)] if echo else [])
        medium = LiveMedium(1, 1, links, device=DEV, max_delay=10)
        assert medium.delayed and medium.hist_len == 16
        tl = timeline(medium)
        row = np.concatenate([expect(tl, medium, host[:, p: p + T], T) for p in range(0, total, T)], axis=1)[0]
        rows[echo] = row
        bursts, _ = O.gate_stream(row, 18000, 14000, 16)
        assert len(bursts) == 1
        want = [O.load_frames(row[s: s + n], 1200) for s, n in bursts]
        print("echo" if echo else "direct", bursts, want)
        rx = LiveReceiver(1, 40, max_burst_len=65536, max_chunk_len=T, device=DEV)
        chunk = torch.zeros((1, T), dtype=torch.int16, device=DEV)
        heard = [[]]
        for p in range(0, total, T):
            medium.mix(src[:, p: p + T], out=chunk)
            same(chunk, row[None, p: p + T], (echo, p))
            collect(rx.push(chunk), heard)
        collect(rx.flush(), heard)
        torch.cuda.synchronize()
        rx.close()
        assert [(g["start"], g["len"]) for g in heard[0]] == bursts
        assert [g["bytes"] for g in heard[0]] == want
        if not echo:
            assert want == [payload] and heard[0][0]["status"] == _native.ST_OK and (row == host[0]).all()
    x = host[0].astype(np.int64)
    late = np.concatenate([np.zeros(10, np.int64), x[:-10]])
    assert (rows[True] == np.clip(x + (late >> 1), -32768, 32767)).all() and (rows[True] != rows[False]).any()


# ----------------------------------------------------------------------------------------------- 9. a carrier that is late

LC_T, LC_TICKS, LC_DELAY = 2048, 22, 4096
LC_A, LC_B = 2, 3                                                  # the ticks at which A and B get their message
LC_HOLDOFF = 4800
LC_TR = afskmodem.Transmitter(1200, 0.05)
LC_PAY = [b"station A calls!", b"station B calls!"]                 # 16 bytes: on air for more than four ticks


def late_carrier_links(delay):
    """Sources: A, B.  Row 0: what A hears (B), row 1: what B hears (A), row 2: a bystander next to both."""
    return [(0, 1, U, delay), (1, 0, U, delay), (2, 0, U, 0), (2, 1, U, 0)]


def late_carrier_model(delay):
    """The ticks on the host models: per tick (medium [3, T], busy [2], samples [2, T], deferred [2])."""
    st = [H.HoldTxModel(1, 40, LC_TR.ts_cycles, 4, 16, wav=LC_TR.wav_samples) for _ in range(2)]
    gates = [H.BusyModel() for _ in range(2)]
    links = late_carrier_links(delay)
    tables = (*medium_csr(3, links), medium_delays(3, links))
    tl = D.Timeline(2, 4096)
    chunk = np.zeros((3, LC_T), np.int16)
    ticks = []
    for t in range(LC_TICKS):
        for s, at in enumerate((LC_A, LC_B)):
            if t == at:
                assert not st[s].submit([0], [LC_PAY[s]])[0].any()
        busy = [gates[s].push(chunk[s]) for s in range(2)]
        pulls = [st[s].pull_hold(LC_T, hold=[busy[s]], holdoff=LC_HOLDOFF) for s in range(2)]
        samples = np.concatenate([p[0] for p in pulls])
        chunk = tl.mix(samples, *tables, 3, LC_T)
        ticks.append((chunk, busy, samples, [int(p[2][0]) for p in pulls]))
    return ticks


def on_air(samples):
    """(first, last + 1) column of each station's tones over the whole run."""
    out = []
    for s in range(2):
        nz = np.nonzero(np.concatenate([t[s] for t in samples]))[0]
        out.append((int(nz[0]), int(nz[-1]) + 1))
    return out


def late_carrier_gpu(torch, delay):
    medium = LiveMedium(2, 3, late_carrier_links(delay), device=DEV, max_delay=LC_DELAY)
    rx = [LiveReceiver(1, 40, max_burst_len=None, max_chunk_len=LC_T, max_payload_len=16, device=DEV) for _ in range(2)]
    tx = [LiveTransmitter(1, 1200, 0.05, queue_depth=4, max_payload_len=16, device=DEV) for _ in range(2)]
    res = [r.alloc_result() for r in rx]
    busy = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2)]
    src = torch.zeros((2, LC_T), dtype=torch.int16, device=DEV)
    chunk = torch.zeros((3, LC_T), dtype=torch.int16, device=DEV)
    ticks = []
    for t in range(LC_TICKS):
        for s, at in enumerate((LC_A, LC_B)):
            if t == at:
                assert (tx[s].submit([0], [LC_PAY[s]]).cpu()[0] == Q).all()
        deferred = []
        for s in range(2):
            rx[s].push(chunk[s: s + 1], out=res[s])
            rx[s].busy(out=busy[s])
        for s in range(2):
            tx[s].pull(LC_T, out=src[s: s + 1], hold=busy[s], holdoff=LC_HOLDOFF)
            deferred.append(int(tx[s].deferred.cpu()[0]))
        medium.mix(src, out=chunk)
        ticks.append((chunk.cpu().numpy().copy(), [int(b.cpu()[0]) for b in busy], src.cpu().numpy().copy(), deferred))
    torch.cuda.synchronize()
    for x in rx + tx:
        x.close()
    return ticks


@pytest.fixture(scope="module")
def late_carrier_models():
    return {d: late_carrier_model(d) for d in (0, LC_DELAY)}


def late_carrier_outcome(ticks):
    samples = [t[2] for t in ticks]
    (a0, a1), (b0, b1) = on_air(samples)
    b_deferred = sum(t[3][1] for t in ticks)
    third = np.concatenate([t[0][2] for t in ticks])
    both = np.concatenate([t[2] for t in ticks], axis=1).astype(np.int64)
    assert (third == np.clip(both[0] + both[1], -32768, 32767)).all()   # the bystander: clip(A + B), column by column
    return (a0, a1), (b0, b1), b_deferred, both


@pytest.mark.parametrize("delay", [0, LC_DELAY])
def test_a_carrier_that_arrives_4096_samples_late_is_not_sensed_in_time(torch_cuda, late_carrier_models, delay):
    """Two carrier-sensing stations at unity, B's message one tick after A's.  At delay 0 (the control) B hears A's
    first block before its own pull and waits until A is done: ``deferred > 0``, the tones never share a column.  With
    4096 samples between them B hears nothing yet, starts at once (``deferred == 0``) and talks over A.  Both outcomes
    are asserted on the host models and on the device, whose every tick equals the models'."""
    model = late_carrier_models[delay]
    (a0, a1), (b0, b1), b_deferred, both = late_carrier_outcome(model)
    assert 0 <= a0 - LC_A * LC_T < 8                                   # A keys up with the pull of its submit tick
    if delay == 0:
        assert b_deferred > 0 and b0 >= a1 and not ((both[0] != 0) & (both[1] != 0)).any()
        assert model[LC_B][1] == [0, 1]                                # B is busy at its submit tick: it heard A
    else:
        assert b_deferred == 0 and 0 <= b0 - LC_B * LC_T < 8 and min(a1, b1) - b0 > 3 * LC_T
        assert ((both[0] != 0) & (both[1] != 0)).sum() > 2 * LC_T      # both on air for more than three ticks
        assert model[LC_B][1] == [0, 0] and model[LC_B + 1][1] == [0, 0] and model[LC_B + 2][1] == [0, 1]
        assert model[LC_B + 3][1] == [1, 1]                            # ... the carriers arrive two ticks late
    got = late_carrier_gpu(torch_cuda, delay)
    for t, (g, w) in enumerate(zip(got, model)):
        for name, x, y in zip(("medium", "busy", "samples", "deferred"), g, w):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (delay, t, name)
    assert late_carrier_outcome(got)[:3] == ((a0, a1), (b0, b1), b_deferred)


# ------------------------------------------------------------------------------------------------------ 10. one graph

T_G, TICKS_G = 4096, 12


def test_a_station_tick_with_a_delayed_noisy_medium_replays_as_one_graph(torch_cuda):
    """push -> busy -> submit_events -> pull(out=src rows, hold=busy, ...) -> medium.mix(src, out=chunk) with delays and
    noise, captured once and replayed: the position and the history advance INSIDE the graph, so every replayed tick
    equals the eager run, whose medium rows are the model's."""
    torch = torch_cuda
    n = 4
    burst = afskmodem.Transmitter(1200, 0.25).wav_samples(bytes(range(65, 89)))
    host = np.zeros((n, TICKS_G * T_G), np.int16)
    host[1, 300: 300 + burst.size] = burst
    dev = torch.from_numpy(host).to(DEV)
    scale = synth.snr_to_scale_q24(40.0)
    kw = dict(holdoff=4800, persist=63, slot=4800, seed=77)

    def station():
        rx = LiveReceiver(n, 40, max_burst_len=65536, max_chunk_len=T_G, device=DEV)
        tx = LiveTransmitter(n, 1200, 0.1, queue_depth=4, max_payload_len=64, device=DEV)
        src = torch.zeros((2 * n, T_G), dtype=torch.int16, device=DEV)     # the station's rows | the capture's
        # (the station hears itself a quarter as loud, 0.1 s late: below its gate, so it relays once)
        medium = LiveMedium.from_matrix([[0.25]], n, extra=1, delay=[[4800, 0.01]], device=DEV, noise_scale_q24=scale,
                                        seed=5)
        assert medium.delayed and medium.hist_len == 8192 and medium.link_delay.tolist() == [4800, 480] * n
        return (rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(n * rx.slots),
                torch.zeros(n, dtype=torch.int32, device=DEV), src, medium,
                torch.zeros((n, T_G), dtype=torch.int16, device=DEV))

    def tick(rx, tx, res, ev, sub, busy, src, medium, chunk, stream=None):
        rx.push(chunk, out=res, events=ev, stream=stream)
        rx.busy(out=busy, stream=stream)
        tx.submit_events(ev, out=sub, stream=stream)
        tx.pull(T_G, out=src[:n], hold=busy, stream=stream, **kw)
        medium.mix(src, out=chunk, stream=stream)

    def snap(sub, busy, src, chunk, tx):
        return tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, busy, src[:n], chunk,
                                                      tx.pending, tx.deferred, tx.on_air))

    rx, tx, res, ev, sub, busy, src, medium, chunk = station()
    tl = timeline(medium)
    eager = []
    for t in range(TICKS_G):
        src[n:].copy_(dev[:, t * T_G:(t + 1) * T_G])
        tick(rx, tx, res, ev, sub, busy, src, medium, chunk)
        eager.append(snap(sub, busy, src, chunk, tx))
        same(chunk, expect(tl, medium, src.cpu().numpy(), T_G), ("medium", t))
    assert medium.pos == TICKS_G * T_G
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    assert sum(int((e[0] == Q).sum()) for e in eager) >= 1 and any(e[4][1].any() for e in eager)   # heard and relayed
    keep = medium                                                   # (the eager run's history, held against the replay's)

    rx, tx, res, ev, sub, busy, src, medium, chunk = station()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):              # one linear chain
            tick(rx, tx, res, ev, sub, busy, src, medium, chunk, stream=side)
    torch.cuda.synchronize()
    tx.reset()                                                  # (the capture ran nothing; start from a clean state)
    rx.reset()
    src.zero_()
    chunk.zero_()
    tx.on_air.zero_()
    medium.reset()
    torch.cuda.synchronize()
    names = ("status", "start", "n_samples", "busy", "samples", "medium", "pending", "deferred", "on_air")
    for t in range(TICKS_G):
        src[n:].copy_(dev[:, t * T_G:(t + 1) * T_G])
        graph.replay()
        for g, w, name in zip(snap(sub, busy, src, chunk, tx), eager[t], names):
            assert (g == w).all(), (t, name)
    assert medium.pos == TICKS_G * T_G
    assert torch.equal(medium.d_history, keep.d_history)
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# ---------------------------------------------------------------------------------------------------- 11. refusals

def test_wrong_arguments_raise_on_the_host_before_anything_is_launched(torch_cuda):
    torch = torch_cuda
    medium = LiveMedium(3, 2, [(0, 0, U, 4), (1, 2, U, 0.0001)], device=DEV)
    assert medium.delayed and medium.max_delay == 5 and medium.hist_len == 8 and medium.history_bytes == 48
    assert medium.link_delay.tolist() == [4, 5]
    buf = torch.full((5, 64), 9, dtype=torch.int16, device=DEV)
    src, out = buf[:3], buf[3:]
    for bad in (dict(src=buf[:2]), dict(src=src.to(torch.int32)), dict(src=src.cpu()), dict(src=src, T=65),
                dict(src=src, out=buf[3:4]), dict(src=src, out=buf[2:4]), dict(src=src, out=buf[3:, ::2], T=32),
                dict(src=src, lengths=[1, 2]), dict(src=src, T=-1), dict(src=medium.d_history.view(3, 8), T=8),
                dict(src=src, out=medium.d_history.view(-1)[:16].view(2, 8), T=8)):
        with pytest.raises((ValueError, TypeError, _native.AfskNativeError)):
            medium.mix(**{"out": out, **bad})
    assert bool((buf == 9).all()) and medium.pos == 0 and not bool(medium.d_history.any())
    assert medium.mix(src, T=0, out=out).shape == (2, 0) and bool((buf == 9).all()) and medium.pos == 0
    with pytest.raises(ValueError):
        medium.reset(-1)
    with pytest.raises(ValueError):
        LiveMedium(3, 2, [(0, 0, U, 9)], device=DEV, max_delay=8)
    with pytest.raises(_native.AfskNativeError, match="delay of -1"):
        LiveMedium(3, 2, [(0, 0, U, -1)], device=DEV)
    medium.reset(12)                                                 # a delayed medium keeps a position without noise
    assert medium.pos == 12
    got = medium.mix(src, out=out)
    assert medium.pos == 76 and bool((got[0, :4] == 0).all()) and bool((got[0, 4:] == 9).all())
    # a medium that is not delayed is what it was: no history, no delay table, no position without noise
    plain = LiveMedium(3, 2, [(0, 0, U), (1, 2, U, 0)], device=DEV, max_delay=0)
    assert not plain.delayed and plain.hist_len == 0 and plain.history_bytes == 0
    assert plain.d_history is None and plain.d_link_delay is None and plain.d_pos is None
    assert afskmodem.LiveMedium is LiveMedium
