"""GPU parity (-m gpu) of both gates with block amplitudes exactly ON their thresholds: the batched gate
(``gate_batch``: block_amp_kernel + gate_scan_kernel) and the live walk (``LiveReceiver``: stored, streaming and
progressive, in its plain, per-channel-threshold and ragged forms) against

  (a) the reference's own listen recordings whose blocks sit on a threshold (tests/golden/reference_listen_edges.json,
      the ``listen_cases`` behind the sixteen of the main fixture: ref:306 opens on amp > amp_start, ref:316 closes on
      amp < amp_end, ref:94-98 truncates and counts -32768 as 32768), and
  (b) - (d) the CPU oracle's whole-capture gate (``O.gate_stream``) on inputs of tests/gate_edge_inputs.py: every
      six-block sequence over the five amplitudes around a pair, and blocks that reach 18001 only if one given sample
      was summed.

Integer paths: every comparison is exact.  The payloads of these square waves are not looked at."""
import numpy as np
import pytest

from afskmodem_amd import _native, batch
from afskmodem_amd.live import LiveReceiver
from oracle import afsk_oracle as O
from tests import gate_edge_inputs as E
from tests.golden_inputs import build_capture, listen_cases
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = E.BLOCK
KINDS = ("stored", "stream", "progressive")
N_RECORDED_BEFORE = 16                                  # the eight captures at two pairs that came first
EDGE_CASES = ("start_at_threshold-18000-14000", "amp_truncates-18000-14000", "full_scale_negative-32767-14000",
              "full_scale_negative-32768-14000", "inverted_pair-14000-18000", "equal_pair-16000-16000",
              "zero_thresholds-0-0", "zero_thresholds-0-1", "densest_at_threshold-18000-14000")


def receiver(kind, n, amp_start, amp_end, T, max_burst_len=6 * BLOCK):
    """A receiver of ``kind`` at 1200 baud; amp_start / amp_end: one value or one per channel."""
    as_arg = lambda v: int(v) if np.ndim(v) == 0 else [int(x) for x in v]  # noqa: E731
    if kind == "stored":
        return LiveReceiver(n, 40, as_arg(amp_start), as_arg(amp_end), max_burst_len=max_burst_len, max_chunk_len=T,
                            device=DEV)
    return LiveReceiver(n, 40, as_arg(amp_start), as_arg(amp_end), max_burst_len=None, max_chunk_len=T, device=DEV,
                        max_payload_len=0 if kind == "progressive" else 16, progressive=kind == "progressive")


def slot_events(res) -> np.ndarray:
    """int64 [m, 4]: (channel, start, len, flags) of the bursts one push reported, from n_closed and the slot arrays
    (synchronises)."""
    nc, bs, bl, fl = (t.cpu().numpy() for t in (res.n_closed, res.burst_start, res.burst_len, res.flags))
    assert nc.min() >= 0 and nc.max() <= res.slots
    c, k = np.nonzero(np.arange(res.slots)[None, :] < nc[:, None])
    return np.stack([c, bs[c, k], bl[c, k], fl[c, k]], axis=1).astype(np.int64)


def packed_events(res) -> np.ndarray:
    """The same table from the push's packed event list (``push(events=...)``)."""
    ev = res.events
    h = ev.header()
    assert h["count"] == h["stored"] == int(res.n_closed.sum())
    r = ev.records()
    return np.stack([r["channel"], r["burst_start"], r["burst_len"], r["flags"]], axis=1).astype(np.int64)


def in_channel_order(tables) -> np.ndarray:
    """The tables of consecutive pushes as one, channel by channel in time order."""
    t = np.concatenate(tables) if tables else np.zeros((0, 4), np.int64)
    return t[np.argsort(t[:, 0], kind="stable")]


def assert_events(got, want, tag):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    chans = np.union1d(got[:, 0], want[:, 0])
    for c in chans.tolist():
        g, w = got[got[:, 0] == c, 1:].tolist(), want[want[:, 0] == c, 1:].tolist()
        assert g == w, (tag, "channel", c, "got (start, len, flags)", g, "want", w)
    raise AssertionError((tag, got.shape, want.shape))


def drive(rx, d, T, packed=False):
    """Push the column windows of d ([n, L] device) of width T, flush with the last one -> the events table."""
    total = d.shape[1]
    ev = rx.alloc_events() if packed else None
    tables = []
    for p in range(0, total, T):
        res = rx.push(d[:, p: p + T], flush=p + T >= total, events=ev)
        tables.append(packed_events(res) if packed else slot_events(res))
    return in_channel_order(tables)


def drive_ragged(torch, rx, d, T, schedule, packed=False):
    """Ragged pushes: at tick i channel c appends the next min(schedule(i)[c], rest of its row) samples of its row,
    from a chunk whose columns behind that count are loud garbage, and is flushed by the mask of the tick that
    finishes its row.  schedule(i) -> int [n] from 0 ... T."""
    n, total = d.shape
    padded = torch.zeros((n, total + T), dtype=torch.int16, device=DEV)
    padded[:, :total] = d
    cols = torch.arange(T, device=DEV)
    pos = np.zeros(n, np.int64)
    ev = rx.alloc_events() if packed else None
    tables, tick = [], 0
    while (pos < total).any():
        lens = np.minimum(np.asarray(schedule(tick), np.int64), total - pos).astype(np.int32)
        assert lens.min() >= 0 and lens.max() <= T
        last = (lens > 0) & (pos + lens == total)
        chunk = torch.gather(padded, 1, torch.from_numpy(pos).to(DEV)[:, None] + cols[None, :])
        chunk.masked_fill_(cols[None, :] >= torch.from_numpy(lens).to(DEV)[:, None], 32767)
        res = rx.push(chunk, lengths=lens, flush=last.astype(np.uint8), events=ev)
        tables.append(packed_events(res) if packed else slot_events(res))
        pos += lens
        tick += 1
        assert tick < 64
    return in_channel_order(tables)


@pytest.fixture(scope="module")
def device_rows(torch_cuda):
    """pair -> the [15625, 12288] device buffer of E.live_rows(pair), uploaded once per module."""
    torch = torch_cuda
    cache = {}

    def get(pair):
        if pair not in cache:
            cache[pair] = torch.from_numpy(E.live_rows(pair)).to(DEV)
        return cache[pair]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------ (a) the reference's recordings

def edge_case(golden, i):
    cases = listen_cases(golden)
    assert len(cases) == N_RECORDED_BEFORE + len(EDGE_CASES)
    c = cases[N_RECORDED_BEFORE + i]
    assert f'{c["name"]}-{c["amp_start"]}-{c["amp_end"]}' == EDGE_CASES[i]
    return c, build_capture(c["recipe"])


@pytest.mark.parametrize("i", range(len(EDGE_CASES)), ids=EDGE_CASES)
def test_recorded_threshold_cases_through_gate_batch(golden, torch_cuda, i):
    torch = torch_cuda
    c, cap = edge_case(golden, i)
    nblk = len(cap) // BLOCK
    want = [(b["start"], b["len"]) for b in c["bursts"]]
    # behind two other captures, so that the capture starts at an odd offset and its slots are not slot 0
    caps = [np.full(4097, 32767, np.int16), cap, np.full(2048, -32768, np.int16)]
    samples, off, ln, max_len = batch.upload_streams(caps)
    for mb in (16, 1):
        g = batch.gate_batch(samples, off, ln, max_len, c["amp_start"], c["amp_end"], mb, slots=True)
        plain = batch.gate_batch(samples, off, ln, max_len, c["amp_start"], c["amp_end"], mb, slots=False)
        torch.cuda.synchronize()
        assert plain.slot_len is None and plain.slot_offset is None
        for res in (g, plain):
            nb, bs, bl, oe, amp = (t.cpu().numpy() for t in (res.n_bursts, res.burst_start, res.burst_len,
                                                              res.open_end, res.block_amp))
            assert amp[1, :nblk].tolist() == c["block_amp"], mb
            assert [(int(bs[1, k]), int(bl[1, k])) for k in range(nb[1])] == want[:mb], mb
            assert int(oe[1]) == (c["open_end"] if len(want) <= mb else 0), mb
            assert (want[:mb], int(oe[1])) == O.gate_stream(cap, c["amp_start"], c["amp_end"], mb)
        s_off, s_len = plain.burst_slots(off)                          # torch arithmetic on the plain outputs
        assert torch.equal(g.slot_offset.reshape(-1), s_off) and torch.equal(g.slot_len.reshape(-1), s_len)
        so, sl = g.slot_offset.cpu().numpy(), g.slot_len.cpu().numpy()
        padded = want[:mb] + [(None, 0)] * (mb - len(want[:mb]))
        assert sl[1].tolist() == [n for _, n in padded]
        assert so[1].tolist() == [0 if s is None else int(off[1]) + s for s, _ in padded]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(EDGE_CASES)), ids=EDGE_CASES)
def test_recorded_threshold_cases_through_the_live_receivers(golden, torch_cuda, i, kind):
    torch = torch_cuda
    c, cap = edge_case(golden, i)
    flags = [0] * (len(c["bursts"]) - c["open_end"]) + [_native.LIVE_OPEN_END] * c["open_end"]
    want = np.array([(0, b["start"], b["len"], f) for b, f in zip(c["bursts"], flags)], np.int64).reshape(-1, 4)
    d = torch.from_numpy(cap.reshape(1, -1).copy()).to(DEV)
    rx = receiver(kind, 1, c["amp_start"], c["amp_end"], len(cap), max_burst_len=65536)
    for T in (2048, 3000, len(cap)):
        assert_events(drive(rx, d, T), want, (EDGE_CASES[i], kind, T))
    assert_events(drive(rx, d, 3000, packed=True), want, (EDGE_CASES[i], kind, "packed"))
    torch.cuda.synchronize()
    rx.close()


# ------------------------------------------------------------------------------ (b) every six-block sequence, batched

@pytest.mark.parametrize("pair", E.PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_every_six_block_sequence_through_gate_batch(torch_cuda, pair):
    torch = torch_cuda
    flat, off, ln = E.flat_captures(pair)
    samples, d_off, d_ln = (torch.from_numpy(a).to(DEV) for a in (flat, off, ln))
    max_len = int(ln.max())
    amps = np.array(E.class_amps(pair))[E.sequences()]
    for mb in (1, 2, 4):
        g = batch.gate_batch(samples, d_off, d_ln, max_len, pair[0], pair[1], mb)
        torch.cuda.synchronize()
        nb, bs, bl, oe, amp, so, sl = (t.cpu().numpy() for t in (g.n_bursts, g.burst_start, g.burst_len, g.open_end,
                                                                  g.block_amp, g.slot_offset, g.slot_len))
        w_nb, w_bs, w_bl, w_oe = E.expected_gate(flat, off, ln, pair, mb)
        assert np.array_equal(amp[:, :6], amps)
        bad = np.nonzero(nb != w_nb)[0]
        assert bad.size == 0, (mb, bad[:5], amps[bad[:5]], nb[bad[:5]], w_nb[bad[:5]])
        assert np.array_equal(oe, w_oe), (mb, np.nonzero(oe != w_oe)[0][:5])
        used = np.arange(mb)[None, :] < w_nb[:, None]
        for name, got, want in (("burst_start", bs, w_bs), ("burst_len", bl, w_bl)):
            bad = np.nonzero(((got != want) & used).any(axis=1))[0]
            assert bad.size == 0, (mb, name, bad[:5], amps[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(sl, w_bl)                                  # zero past n_bursts
        assert np.array_equal(so, np.where(used, off[:, None] + w_bs, 0))
    assert int(w_nb.max()) == 2 and 0 < int(w_oe.sum()) < E.N_SEQ


# ------------------------------------------------------------------------------ (c) the same sequences, live channels

@pytest.mark.parametrize("T", [2048, 3000, 6 * BLOCK])
@pytest.mark.parametrize("kind", KINDS)
def test_every_six_block_sequence_as_live_channels(torch_cuda, device_rows, kind, T):
    pair = (18000, 14000)
    d = device_rows(pair)
    rx = receiver(kind, E.N_SEQ, pair[0], pair[1], T)
    assert rx.amp_start_threshold == pair[0] and rx.amp_end_threshold == pair[1]
    assert_events(drive(rx, d, T, packed=T == 3000), E.expected_live(pair), (kind, T))
    torch_cuda.cuda.synchronize()
    rx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_six_block_sequence_with_per_channel_thresholds(torch_cuda, device_rows, kind):
    """Channels alternate between (18000, 14000) and the inverted (14000, 18000), each fed the class amplitudes of its
    own pair."""
    pa, pb = (18000, 14000), (14000, 18000)
    d = device_rows(pa).clone()
    d[1::2] = device_rows(pb)[1::2]
    odd = np.arange(E.N_SEQ) % 2 == 1
    start, end = np.where(odd, pb[0], pa[0]), np.where(odd, pb[1], pa[1])
    wa, wb = E.expected_live(pa), E.expected_live(pb)
    want = in_channel_order([wa[wa[:, 0] % 2 == 0], wb[wb[:, 0] % 2 == 1]])
    rx = receiver(kind, E.N_SEQ, start, end, 3000)
    assert rx.amp_start_threshold is None and rx.amp_end_threshold is None
    assert_events(drive(rx, d, 3000), want, (kind, "per channel"))
    torch_cuda.cuda.synchronize()
    rx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_six_block_sequence_in_ragged_pushes(torch_cuda, device_rows, kind):
    pair, T = (16000, 16000), 3000
    d = device_rows(pair)
    rng = np.random.default_rng(17)
    sizes = np.array([0, 1, 2047, 2048, 2049, T])

    def schedule(tick):
        return rng.choice(sizes, E.N_SEQ) if tick < 10 else np.full(E.N_SEQ, T)

    rx = receiver(kind, E.N_SEQ, pair[0], pair[1], T)
    assert_events(drive_ragged(torch_cuda, rx, d, T, schedule, packed=True), E.expected_live(pair), (kind, "ragged"))
    torch_cuda.cuda.synchronize()
    rx.close()


# ------------------------------------------------------------------------------ (d) every sample counts

def test_every_sample_reaches_the_block_sum_in_gate_batch(torch_cuda):
    torch = torch_cuda
    rows = E.every_sample_rows()
    n, L = rows.shape
    # one loud sample in front: every capture starts at an odd offset
    flat = np.concatenate([np.full(1, 32767, np.int16), rows.reshape(-1)])
    off = 1 + np.arange(n, dtype=np.int64) * L
    g = batch.gate_batch(torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV),
                         torch.full((n,), L, dtype=torch.int32, device=DEV), L, 18000, 14000, 2)
    torch.cuda.synchronize()
    nb, bs, bl, oe, amp = (t.cpu().numpy() for t in (g.n_bursts, g.burst_start, g.burst_len, g.open_end, g.block_amp))
    opens = np.arange(n) < BLOCK
    assert np.array_equal(amp, np.stack([np.zeros(n), np.where(opens, 18001, 18000), np.zeros(n)], axis=1))
    assert np.array_equal(nb, opens.astype(np.int32)), np.nonzero(nb != opens)[0][:8]
    assert np.all(bs[opens, 0] == BLOCK) and np.all(bl[opens, 0] == 2 * BLOCK) and not oe.any()


def test_every_sample_reaches_the_block_sum_in_the_live_walk(torch_cuda):
    """The deciding block loaded whole from the chunk (T = 2048), at odd chunk offsets behind a carried block, and put
    together from the carry and the chunk at every split point 1 ... 2047."""
    torch = torch_cuda
    rows = E.every_sample_rows()
    n, L = rows.shape
    d = torch.from_numpy(rows).to(DEV)
    want = E.expected_events(rows[: BLOCK + 8], 18000, 14000)          # (the rows that must not open report nothing)
    assert want.tolist() == [[c, BLOCK, 2 * BLOCK, 0] for c in range(BLOCK)]
    rx = receiver("stored", n, 18000, 14000, 3000)
    assert_events(drive(rx, d, 2048), want, "T = 2048")
    assert_events(drive(rx, d, 3000), want, "T = 3000")                # the deciding block: 952 carried samples
    c = np.arange(n)
    for tag, first in (("phases 1 ... 7", 1 + c % 7),                  # ... 953 ... 959 carried samples
                       # a first push of k samples: for k >= 1096 the deciding block is read from the chunk at column
                       # 2048 - k behind a block of k carried samples, below that it has 952 + k carried samples
                       ("carry 1 ... 2047", 1 + (c * 37 + c // BLOCK) % 2047)):
        schedule = lambda tick, first=first: first if tick == 0 else np.full(n, 3000)  # noqa: E731
        assert_events(drive_ragged(torch, rx, d, 3000, schedule), want, tag)
    assert set((1 + (c[:BLOCK] * 37) % 2047).tolist()) == set(range(1, 2048))
    torch.cuda.synchronize()
    rx.close()
