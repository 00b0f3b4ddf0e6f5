"""GPU parity (-m gpu) of the live medium: ``LiveMedium.mix`` (afsk_live_mix: live_mix_kernel and, with noise,
live_mix_advance_kernel) against the numpy model of the header's rule (tests/live_mix_model.py), sample for sample.

Expected values never come from the code under test: the mix is the model's, its noise the CPU oracle's generator (or
the model's numpy restatement of it where the position is out of the oracle's reach).  The last three tests also hold
the medium against existing pieces: the oracle's gate and decoder behind a ``LiveReceiver``, the two-station scenario
of tests/live_csma_scenario.py, and one captured graph of a whole station tick.  Integer samples: every comparison is
exact."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, synth
from afskmodem_amd.live import LiveMedium, LiveReceiver, LiveTransmitter, medium_csr
from oracle import afsk_oracle as O
from tests import live_csma_scenario as S
from tests import live_mix_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import collect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = M.UNITY
POISON = 32767
Q = _native.LIVE_TX_QUEUED


def strided(torch, rows, T, base, fill=0):
    """An int16 [rows, T + 3] view with row stride T + 3 that begins ``base`` samples into a flat buffer of ``fill``
    (``base`` odd: every row begins at an address that is a multiple of 2 and of nothing more), and the buffer."""
    stride = T + 3
    flat = torch.full((base + rows * stride + 5,), fill, dtype=torch.int16, device=DEV)
    return flat.as_strided((rows, stride), (stride, 1), base), flat


def upload(torch, host, view):
    view.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(DEV))


def same(got, want, tag):
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist(), [int(got[tuple(b)]) for b in bad[:4]],
                           [int(want[tuple(b)]) for b in bad[:4]])


def model_of(medium, src, T, lens=None, pos=0):
    """The model over the tables as they lie ON THE DEVICE now."""
    scale = None if medium.d_noise_scale_q24 is None else medium.d_noise_scale_q24.cpu().numpy()
    return M.mix(src, medium.d_row_ptr.cpu().numpy(), medium.d_link_src.cpu().numpy(),
                 medium.d_link_gain_q15.cpu().numpy(), medium.n_out, T, src_lens=lens, noise_scale_q24=scale,
                 seed=medium.seed, noise_idx_base=medium.noise_idx_base, pos=pos)


# ------------------------------------------------------------------------------------- 1. sizes, bases and strides

@pytest.mark.parametrize("T", [1, 7, 8, 9, 2047, 2048, 2049])
def test_every_tail_at_odd_row_bases_and_strides(torch_cuda, T):
    """Rows that begin at odd sample offsets with stride T + 3; out beyond T is poisoned and must stay so; src beyond
    every source's length is poisoned and must not be heard."""
    torch = torch_cuda
    rng = np.random.default_rng(T)
    n_src, n_out = 5, 4
    lens = [T, max(T - 1, 0), T // 2, T + 9, max(T - 8, 0)]
    host = rng.integers(-32768, 32768, (n_src, T + 3), dtype=np.int16)
    for s in range(n_src):
        host[s, max(min(lens[s], T), 0):] = POISON
    src, _ = strided(torch, n_src, T, 1)
    upload(torch, host, src)
    out, flat = strided(torch, n_out, T, 3, fill=POISON)
    links = [(1, 3, U), (2, 0, U // 2), (2, 1, -U // 2), (3, 0, U), (3, 1, U), (3, 2, 0.75), (3, 4, -U), (3, 1, U)]
    medium = LiveMedium(n_src, n_out, links, device=DEV)
    got = medium.mix(src, T, out=out, lengths=lens)
    assert tuple(got.shape) == (n_out, T) and got.data_ptr() == out.data_ptr()
    want = model_of(medium, host, T, lens)
    same(got, want, T)
    assert not want[0].any() and want[1:].any()
    rest = torch.ones_like(flat, dtype=torch.bool)
    rest.as_strided((n_out, T), (T + 3, 1), 3).fill_(False)
    assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
    # the poison WOULD have been heard: the same mix without the lengths differs wherever a row is cut
    if T > 1:
        assert (M.mix(host, medium.row_ptr, medium.link_src, medium.link_gain_q15, n_out, T) != want).any()


# ------------------------------------------------------------------------------ 2. degrees, gains and broken tables

T2 = 2056                                                    # a tile and one thread of the next


def gain_case(torch):
    rng = np.random.default_rng(2)
    host = rng.integers(-32768, 32768, (6, T2), dtype=np.int16)
    host[0], host[1] = 32767, -32768
    host[4] = rng.integers(-3, 4, T2)                         # products around 0: the floor shows
    links = [(1, 0, U), (1, 0, U),                            # a duplicate link: 32767 + 32767
             (2, 1, U), (2, 1, U),                            # -32768 - 32768
             (3, 4, 1),
             (4, 2, 0), (4, 4, 1), (4, 3, -U), (4, 5, U), (4, 2, 65535),
             (5, 0, -65535), (5, 1, -65535),
             (6, 2, -U), (7, 5, 65535), (7, 5, 65535), (8, 4, -1)]
    src = torch.from_numpy(host).to(DEV)
    return host, src, LiveMedium(6, 9, links, device=DEV)


def test_degrees_0_1_2_5_a_duplicate_link_and_every_corner_gain(torch_cuda):
    torch = torch_cuda
    host, src, medium = gain_case(torch)
    assert np.diff(medium.row_ptr).tolist() == [0, 2, 2, 1, 5, 2, 1, 2, 1]
    got = medium.mix(src)
    want = model_of(medium, host, T2)
    same(got, want, "gains")
    assert not want[0].any() and (want[1] == 32767).all() and (want[2] == -32768).all()
    assert set(np.unique(want[3]).tolist()) == {-1, 0}          # (-3 ... 3) * 1 >> 15: floor
    assert (want[5] == -65534 + 65535).all()                      # floor(-65535 * 32767 / 32768) + 65535
    assert (want[6, host[2] == -32768] == 32767).all()           # +32768 clips
    assert (want[7] == 32767).any() and (want[7] == -32768).any()


def test_gains_and_sources_beyond_range_on_the_device_are_clamped_and_ignored(torch_cuda):
    """The tables are overwritten where they lie: the kernel clamps a gain to +-65535 and ignores a link whose source
    lies outside the matrix -- by construction no index reaches a load unclamped."""
    torch = torch_cuda
    host, src, medium = gain_case(torch)
    gains = medium.link_gain_q15.copy()
    gains[[0, 2, 5, 9, 13]] = [70000, -70000, 2 ** 31 - 1, -2 ** 31, 65536]
    medium.d_link_gain_q15.copy_(torch.from_numpy(gains))
    want = model_of(medium, host, T2)
    same(medium.mix(src), want, "gains beyond range")
    assert (want != M.mix(host, medium.row_ptr, medium.link_src, medium.link_gain_q15, 9, T2)).any()
    srcs = medium.link_src.copy()
    srcs[[1, 3, 6, 8, 12]] = [-1, 6, 2 ** 31 - 1, -2 ** 31, 70000]
    medium.d_link_src.copy_(torch.from_numpy(srcs))
    want = model_of(medium, host, T2)
    same(medium.mix(src), want, "sources out of range")
    # one duplicate each is left: 32767 * 65535 >> 15 = 65533 and -32768 * -65535 >> 15 = 65535, both clipped
    assert (want[1] == 32767).all() and (want[2] == 32767).all()
    same(medium.mix(src, lengths=[T2, 5, 0, T2 - 1, 9, T2]), model_of(medium, host, T2, [T2, 5, 0, T2 - 1, 9, T2]),
         "sources out of range, ragged")


def test_a_row_ptr_that_falls_is_an_empty_row(torch_cuda):
    torch = torch_cuda
    host, src, medium = gain_case(torch)
    n = medium.n_links
    for tag, rp in (("falls", [0, 0, 2, 4, 1, 10, 12, 13, 15, 16]),          # row 3 empty; row 4 hears links 1 ... 9
                    ("negative and beyond", [-7, 0, 2, 4, 5, 10, 12, n + 40, 3, n]),
                    ("all beyond", [n + 1] * 10), ("all negative", [-1] * 10),
                    ("int32 corners", [-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 0, n, 0, n, 2 ** 31 - 1, 0])):
        medium.d_row_ptr.copy_(torch.tensor(rp, dtype=torch.int32))
        want = model_of(medium, host, T2)
        same(medium.mix(src), want, tag)
    want = M.mix(host, [0, 0, 2, 4, 1, 10, 12, 13, 15, 16], medium.link_src, medium.link_gain_q15, 9, T2)
    assert not want[3].any() and want[4].any()


# ---------------------------------------------------------------------------------------------- 3. source lengths

@pytest.mark.parametrize("T", [19, 2049])
def test_source_lengths_below_zero_zero_one_T_and_beyond(torch_cuda, T):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    lens = [-5, 0, 1, T, T + 9]
    host = rng.integers(-9000, 9000, (5, T), dtype=np.int16)
    for s, ln in enumerate(lens):
        host[s, max(min(ln, T), 0):] = POISON
    src = torch.from_numpy(host).to(DEV)
    medium = LiveMedium(5, 3, [(0, s, U) for s in range(5)] + [(1, 2, U), (2, 0, U), (2, 1, U)], device=DEV)
    d_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for tag, given in (("host", lens), ("device", d_lens)):
        got = medium.mix(src, lengths=given)
        want = model_of(medium, host, T, lens)
        same(got, want, (T, tag))
    assert want[1, 0] == host[2, 0] and not want[1, 1:].any() and not want[2].any()
    assert (want[0, 1:] == np.clip(host[3, 1:].astype(int) + host[4, 1:], -32768, 32767)).all()


# ------------------------------------------------------------------------------------------- 4. a grid past 65535

def test_70000_output_rows(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(4)
    n_out, n_src, T = 70000, 1000, 8
    host = rng.integers(-32768, 32768, (n_src, T), dtype=np.int16)
    a, b = np.arange(n_out) % n_src, (np.arange(n_out) * 7 + 3) % n_src
    ga, gb = rng.integers(-65535, 65536, n_out), rng.integers(-65535, 65536, n_out)
    links = [(r, s, g) for r in range(n_out) for s, g in ((int(a[r]), int(ga[r])), (int(b[r]), int(gb[r])))]
    medium = LiveMedium(n_src, n_out, links, device=DEV)
    got = medium.mix(torch.from_numpy(host).to(DEV))
    x = host.astype(np.int64)
    want = np.clip(((ga[:, None] * x[a]) >> 15) + ((gb[:, None] * x[b]) >> 15), -32768, 32767).astype(np.int16)
    rows = [0, 1, 65535, 65536, 69999]                            # the rule written out, held against the model
    sel = M.mix(host, *medium_csr(len(rows), [(i, s, g) for i, r in enumerate(rows) for s, g in
                                               ((int(a[r]), int(ga[r])), (int(b[r]), int(gb[r])))]), len(rows), T)
    assert (sel == want[rows]).all()
    same(got, want, "70000 rows")


# ------------------------------------------------------------------------------------------------------- 5. noise

NOISE_T = 4096
SCALES = [1 << 20, 0, 5 << 20, 1 << 27]                          # (the last clips on its own)


def noise_case(torch, **kw):
    rng = np.random.default_rng(5)
    host = rng.integers(-30000, 30000, (3, NOISE_T), dtype=np.int16)
    links = [(0, 0, U), (0, 1, U), (1, 2, 0.5), (2, 0, U), (2, 1, -U), (2, 2, U), (3, 1, 0.25)]
    return host, torch.from_numpy(host).to(DEV), LiveMedium(3, 4, links, device=DEV, noise_scale_q24=SCALES, **kw), links


def test_noise_at_position_0_is_the_noiseless_mix_plus_add_noise_batch(torch_cuda):
    torch = torch_cuda
    host, src, medium, links = noise_case(torch, seed=99, noise_idx_base=1000)
    quiet = LiveMedium(3, 4, links, device=DEV)
    assert quiet.pos == 0 and medium.pos == 0
    got = medium.mix(src)
    plain = quiet.mix(src).contiguous()
    clean = plain.clone()
    same(plain, M.mix(host, medium.row_ptr, medium.link_src, medium.link_gain_q15, 4, NOISE_T), "noiseless")
    assert torch.equal(got[1], plain[1])                          # a scale of 0: the row is untouched
    off, ln = batch.uniform_layout(4, NOISE_T, torch.device(DEV))
    batch.add_noise_batch(plain.view(-1), off, ln, NOISE_T, SCALES, seed=99, stream_idx_base=1000)
    assert torch.equal(got, plain)
    same(got, model_of(medium, host, NOISE_T), "noise at 0")
    assert medium.pos == NOISE_T and quiet.pos == 0
    assert bool((got[3] == 32767).any()) and bool((got[0] != clean[0]).any())


def test_two_ticks_of_2048_equal_one_tick_of_4096(torch_cuda):
    torch = torch_cuda
    host, src, a, links = noise_case(torch, seed=7)
    b = LiveMedium(3, 4, links, device=DEV, noise_scale_q24=SCALES, seed=7)
    whole = a.mix(src)
    halves = torch.cat([b.mix(src[:, :2048]).clone(), b.mix(src[:, 2048:]).clone()], dim=1)
    assert torch.equal(whole, halves) and a.pos == b.pos == NOISE_T
    same(whole, model_of(a, host, NOISE_T), "4096 at once")
    same(b.mix(src[:, :1000]), model_of(b, host[:, :1000], 1000, pos=NOISE_T), "a third tick")
    b.reset()
    assert b.pos == 0
    same(b.mix(src), model_of(b, host, NOISE_T), "after reset")


def test_the_sample_index_wraps_at_2_32(torch_cuda):
    torch = torch_cuda
    host, src, medium, _ = noise_case(torch, seed=11, noise_idx_base=2 ** 32 - 2)     # (the stream index wraps too)
    start = 2 ** 32 - 1000
    medium.reset(start)
    assert medium.pos == start
    got = medium.mix(src[:, :2048])
    want = model_of(medium, host[:, :2048], 2048, pos=start)
    same(got, want, "across the wrap")
    assert medium.pos == start + 2048
    # behind the wrap the noise is that of position 0, as the uint32 index says (the oracle draws it)
    medium.reset()
    same(medium.mix(src[:, 1000:2048]), want[:, 1000:], "position 0")


# ------------------------------------------------------------------------------------- 6. the gain decides the gate

def test_a_listener_at_18100_hears_the_burst_and_one_at_17900_does_not(torch_cuda):
    """One 1200-baud burst, two listeners: at gain_q15 18100 the tones reach 18099 and open the gate (18000), at 17900
    they do not.  The oracle's gate and decoder on the MODEL's rows say what the receiver must report."""
    torch = torch_cuda
    T = 2048
    payload = b"near/far"
    wav = afskmodem.Transmitter(1200, 0.1).wav_samples(payload)
    total = -(-(T + 100 + wav.size + 3 * T) // T) * T
    host = np.zeros((1, total), np.int16)
    host[0, T + 100: T + 100 + wav.size] = wav
    medium = LiveMedium(1, 2, [(0, 0, 18100), (1, 0, 17900)], device=DEV)
    rows = M.mix(host, medium.row_ptr, medium.link_src, medium.link_gain_q15, 2, total)
    assert rows[0].max() == 18099 and rows[1].max() == 17899
    near, _ = O.gate_stream(rows[0], 18000, 14000, 16)
    far, _ = O.gate_stream(rows[1], 18000, 14000, 16)
    assert len(near) == 1 and far == []
    s, n = near[0]
    assert O.load_frames(rows[0, s: s + n], 1200) == payload
    src = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(2, 40, max_burst_len=65536, max_chunk_len=T, device=DEV)
    chunk = torch.zeros((2, T), dtype=torch.int16, device=DEV)
    heard = [[], []]
    for p in range(0, total, T):
        medium.mix(src[:, p: p + T], out=chunk)
        same(chunk, rows[:, p: p + T], p)
        collect(rx.push(chunk), heard)
    collect(rx.flush(), heard)
    torch.cuda.synchronize()
    rx.close()
    assert heard[1] == []
    assert [(g["start"], g["len"]) for g in heard[0]] == near
    assert heard[0][0]["status"] == _native.ST_OK and heard[0][0]["bytes"] == payload


# -------------------------------------------------------------------------------- 7. two stations on one channel

class MixStation:
    """One half-duplex station of the scenario whose pull writes its rows of the medium's source matrix in place."""

    def __init__(self, torch, seed, rows):
        self.rx = LiveReceiver(S.PAIRS, 40, max_burst_len=None, max_chunk_len=S.T, max_payload_len=S.MAXP, device=DEV)
        self.tx = LiveTransmitter(S.PAIRS, 1200, 0.05, queue_depth=S.DEPTH, max_payload_len=S.MAXP, device=DEV)
        self.res = self.rx.alloc_result()
        self.busy = torch.zeros(S.PAIRS, dtype=torch.int32, device=DEV)
        self.last = rows
        self.seed = seed

    def close(self):
        self.rx.close()
        self.tx.close()


def drive_two_stations(torch, persist, slot):
    run = S.run(S.CsmaScenario(persist, slot, (S.SEED_A, S.SEED_B)))
    assert run.done and len(run.medium) <= 60
    P = S.PAIRS
    third = torch.from_numpy(S.third_samples()).to(DEV)
    src = torch.zeros((3 * P, S.T), dtype=torch.int16, device=DEV)          # station A | station B | the third sender
    medium = LiveMedium.from_matrix([[1.0, 1.0]], P, extra=1, device=DEV)
    assert (medium.n_src, medium.n_out) == (3 * P, P) and np.diff(medium.row_ptr).tolist() == [3] * P
    assert (medium.link_gain_q15 == U).all()
    chunk = torch.zeros((P, S.T), dtype=torch.int16, device=DEV)
    st = [MixStation(torch, S.SEED_A, src[0:P]), MixStation(torch, S.SEED_B, src[P: 2 * P])]
    monitor = LiveReceiver(P, 40, max_burst_len=None, max_chunk_len=S.T, max_payload_len=S.MAXP, device=DEV)
    heard = [[] for _ in range(P)]
    for t in range(len(run.medium)):
        if t == S.SUBMIT_TICK:
            for s, x in enumerate(st):
                assert (x.tx.submit(list(range(P)), S.PAY[s]).cpu()[0] == Q).all()
        src[2 * P:].copy_(third[:, t * S.T:(t + 1) * S.T])
        medium.mix(src, out=chunk)
        same(chunk, run.medium[t], ("medium", t))
        collect(monitor.push(chunk), heard)
        for s, x in enumerate(st):
            x.rx.push(chunk, out=x.res, mute=x.tx.on_air)
            x.rx.busy(out=x.busy)
            assert x.busy.tolist() == run.busy[t][s], ("busy", t, s)
        for s, x in enumerate(st):
            x.tx.pull(S.T, out=x.last, hold=x.busy, holdoff=S.HOLDOFF, persist=persist, slot=slot, seed=x.seed)
            same(x.last, run.samples[t][s], ("samples", t, s))
            for name, got in (("pending", x.tx.pending), ("deferred", x.tx.deferred), ("on_air", x.tx.on_air)):
                assert (got.cpu().numpy() == getattr(run, name)[t][s]).all(), (name, t, s)
    collect(monitor.flush(), heard)
    torch.cuda.synchronize()
    for x in st:
        x.close()
    monitor.close()
    return run, [{r["bytes"] for r in rows if r["status"] == _native.ST_OK} for rows in heard]


def test_two_stations_collide_through_the_medium(torch_cuda):
    run, decoded = drive_two_stations(torch_cuda, 255, 0)
    assert run.starts[0] == run.starts[1] == [S.start_when_released()] * S.PAIRS
    for c in range(S.PAIRS):
        assert b"thirdone" in decoded[c], c
        assert S.PAY[0][c] not in decoded[c] and S.PAY[1][c] not in decoded[c], c


def test_two_stations_take_turns_through_the_medium(torch_cuda):
    run, decoded = drive_two_stations(torch_cuda, 63, 4800)
    assert {a < b for a, b in zip(*run.starts)} == {True, False}
    for c in range(S.PAIRS):
        assert {b"thirdone", S.PAY[0][c], S.PAY[1][c]} <= decoded[c], (c, decoded[c])


# ------------------------------------------------------------------------------------------------------ 8. one graph

T_G, TICKS_G = 8192, 20


def test_a_station_tick_with_its_medium_replays_as_one_graph(torch_cuda):
    """push(events=, mute=tx.on_air) -> busy -> submit_events -> pull(out=src rows, hold=busy, ...) ->
    medium.mix(src, out=chunk), captured once and replayed with the capture's rows rewritten between replays.  The
    medium has noise, so the position must advance INSIDE the graph: every tick of the replay equals the eager run,
    whose medium rows are the model's."""
    torch = torch_cuda
    n = 4
    burst = afskmodem.Transmitter(1200, 0.5).wav_samples(bytes(range(65, 89)))
    host = np.zeros((n, TICKS_G * T_G), np.int16)
    host[1, 300: 300 + burst.size] = burst
    dev = torch.from_numpy(host).to(DEV)
    scale = synth.snr_to_scale_q24(40.0)
    kw = dict(holdoff=4800, persist=63, slot=4800, seed=77)

    def station():
        rx = LiveReceiver(n, 40, max_burst_len=65536, max_chunk_len=T_G, device=DEV)
        tx = LiveTransmitter(n, 1200, 0.1, queue_depth=4, max_payload_len=64, device=DEV)
        src = torch.zeros((2 * n, T_G), dtype=torch.int16, device=DEV)     # the station's rows | the capture's
        medium = LiveMedium.from_matrix([[1.0]], n, extra=1, device=DEV, noise_scale_q24=scale, seed=5)
        return (rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(n * rx.slots),
                torch.zeros(n, dtype=torch.int32, device=DEV), src, medium,
                torch.zeros((n, T_G), dtype=torch.int16, device=DEV))

    def tick(rx, tx, res, ev, sub, busy, src, medium, chunk, stream=None):
        rx.push(chunk, out=res, events=ev, mute=tx.on_air, stream=stream)
        rx.busy(out=busy, stream=stream)
        tx.submit_events(ev, out=sub, stream=stream)
        tx.pull(T_G, out=src[:n], hold=busy, stream=stream, **kw)
        medium.mix(src, out=chunk, stream=stream)

    def snap(sub, busy, src, chunk, tx):
        return tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, busy, src[:n], chunk,
                                                      tx.pending, tx.deferred, tx.on_air))

    rx, tx, res, ev, sub, busy, src, medium, chunk = station()
    eager = []
    for t in range(TICKS_G):
        src[n:].copy_(dev[:, t * T_G:(t + 1) * T_G])
        tick(rx, tx, res, ev, sub, busy, src, medium, chunk)
        eager.append(snap(sub, busy, src, chunk, tx))
        same(chunk, model_of(medium, src.cpu().numpy(), T_G, pos=t * T_G), ("medium", t))
    assert medium.pos == TICKS_G * T_G
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    assert sum(int((e[0] == Q).sum()) for e in eager) == 1         # heard once, relayed once: it mutes its own relay
    assert any(e[4][1].any() for e in eager) and sum(int(e[3][1]) for e in eager) >= 2

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
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# ---------------------------------------------------------------------------------------------------- 9. refusals

def test_wrong_arguments_raise_before_anything_is_launched(torch_cuda):
    torch = torch_cuda
    medium = LiveMedium(3, 2, [(0, 0, U), (1, 2, U)], device=DEV)
    buf = torch.full((5, 64), 9, dtype=torch.int16, device=DEV)
    src, out = buf[:3], buf[3:]
    for bad in (dict(src=buf[:2]), dict(src=src.to(torch.int32)), dict(src=src.cpu()), dict(src=src, T=65),
                dict(src=src, out=buf[3:4]), dict(src=src, out=buf[2:4]), dict(src=src, out=buf[3:, ::2], T=32),
                dict(src=src, lengths=[1, 2]), dict(src=src, T=-1)):
        with pytest.raises((ValueError, TypeError, _native.AfskNativeError)):
            medium.mix(**{"out": out, **bad})
    assert bool((buf == 9).all())
    with pytest.raises(ValueError):
        medium.reset(5)
    assert medium.mix(src, T=0, out=out).shape == (2, 0) and bool((buf == 9).all())
    got = medium.mix(src, out=out)
    assert bool((got == 9).all()) and medium.pos == 0
    assert afskmodem.LiveMedium is LiveMedium


# ----------------------------------------------------------------------------------------- 10. the header's limits

T_LIMIT = 2049                                                   # a tile and the first column of the next


def test_a_row_of_32768_links_reaches_2147450880_and_a_balanced_one_returns_to_its_source(torch_cuda):
    """The header promises that a row's sum fits int32 at 32768 links of gain +-65535: row 0 reaches that sum on a
    source held at -32768 and clips; row 1 climbs half as high, comes back down and ends as its one unity source -- the
    sum neither wrapped nor saturated on the way.  Rows at odd bases, the output beyond T poisoned."""
    torch = torch_cuda
    n_src, n_out, links = M.limit_links()
    rng = np.random.default_rng(10)
    host = np.stack([np.full(T_LIMIT + 3, -32768, np.int16), rng.integers(-32768, 32768, T_LIMIT + 3, dtype=np.int16)])
    src, _ = strided(torch, n_src, T_LIMIT, 1)
    upload(torch, host, src)
    out, flat = strided(torch, n_out, T_LIMIT, 3, fill=POISON)
    medium = LiveMedium(n_src, n_out, links, device=DEV)
    assert np.diff(medium.row_ptr).tolist() == [M.MAX_DEGREE, M.MAX_DEGREE]
    got = medium.mix(src, T_LIMIT, out=out)
    want = model_of(medium, host, T_LIMIT)
    same(got, want, "the limit rows")
    assert (want[0] == 32767).all() and (want[1] == host[1, :T_LIMIT]).all()
    rest = torch.ones_like(flat, dtype=torch.bool)
    rest.as_strided((n_out, T_LIMIT), (T_LIMIT + 3, 1), 3).fill_(False)
    assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"


@pytest.mark.parametrize("span", [M.MAX_DEGREE + 1, 40000])
def test_a_row_ptr_span_above_32768_counts_the_first_32768_links(torch_cuda, span):
    """``row_ptr[1]`` is overwritten where it lies.  The link arrays hold every entry up to it (row 1's links follow row
    0's), so the kernel that forgot the clamp would add source 3 to row 0 -- a wrong sum, not a read out of bounds."""
    torch = torch_cuda
    n_src, n_out, links = M.span_links()
    rng = np.random.default_rng(11)
    host = rng.integers(-32768, 32768, (n_src, T_LIMIT), dtype=np.int16)
    host[3] = np.where(np.abs(host[3]) < 4, 400, host[3])       # a quarter of it is never 0
    src = torch.from_numpy(host).to(DEV)
    medium = LiveMedium(n_src, n_out, links, device=DEV)
    n = medium.n_links
    assert medium.row_ptr.tolist() == [0, M.MAX_DEGREE, n] and span <= n == int(medium.d_link_src.numel())
    medium.d_row_ptr.copy_(torch.tensor([0, span, n], dtype=torch.int32))
    want = model_of(medium, host, T_LIMIT)
    same(medium.mix(src), want, span)
    assert (want[0] == host[1]).all()                             # its first 32768 links, and no more
    one_more = (M.UNITY // 4 * host[3].astype(np.int64)) >> 15
    assert (one_more != 0).all()


def test_two_rows_of_2_20_columns(torch_cuda):
    torch = torch_cuda
    T = 1 << 20
    host = np.random.default_rng(12).integers(-32768, 32768, (1, T), dtype=np.int16)
    medium = LiveMedium(1, 2, [(0, 0, U), (1, 0, -U // 2)], device=DEV)
    got = medium.mix(torch.from_numpy(host).to(DEV))
    assert tuple(got.shape) == (2, T)
    same(got, model_of(medium, host, T), "2^20 columns")
    with pytest.raises(ValueError):
        medium.mix(torch.zeros((1, T + 1), dtype=torch.int16, device=DEV))


def test_a_source_length_at_every_residue_around_every_tile_edge(torch_cuda):
    """T = 3 * 2048 - 3; source s ends at 2048 t + d, t in 0 ... 2, d in -9 ... 9 (below 0: silent).  Every source has
    a unity row of its own, one more row hears them all; the sources are poisoned from their length on."""
    torch = torch_cuda
    T = 3 * 2048 - 3
    lens = [2048 * t + d for t in range(3) for d in range(-9, 10)]
    n = len(lens)
    rng = np.random.default_rng(13)
    host = rng.integers(-32768, 32768, (n, T + 3), dtype=np.int16)
    for s, ln in enumerate(lens):
        host[s, max(ln, 0):] = POISON
    src, _ = strided(torch, n, T, 1)
    upload(torch, host, src)
    links = [(s, s, U) for s in range(n)] + [(n, s, U // 64) for s in range(n)]
    medium = LiveMedium(n, n + 1, links, device=DEV)
    out, flat = strided(torch, n + 1, T, 3, fill=POISON)
    got = medium.mix(src, T, out=out, lengths=torch.tensor(lens, dtype=torch.int32, device=DEV))
    want = model_of(medium, host, T, lens)
    same(got, want, "lengths around the tile edges")
    for s, ln in enumerate(lens):
        assert not want[s, max(ln, 0):].any() and (want[s, : max(ln, 0)] == host[s, : max(ln, 0)]).all(), s
    rest = torch.ones_like(flat, dtype=torch.bool)
    rest.as_strided((n + 1, T), (T + 3, 1), 3).fill_(False)
    assert bool((flat[rest] == POISON).all()), "out was written outside its T columns"
