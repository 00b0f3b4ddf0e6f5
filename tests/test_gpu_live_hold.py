"""GPU parity (-m gpu) of carrier sense on the live side: ``LiveTransmitter.pull(hold=, holdoff=)``
(afsk_live_tx_pull_hold: live_tx_tile_hold_kernel*, live_tx_commit_hold_kernel) and ``LiveReceiver.busy``
(afsk_live_busy).

Expected values never come from the code under test.  Samples are ``Transmitter(baud, t).wav_samples(payload)`` -- the
host mirror the golden digests pin to the reference -- placed where the hold model (tests/live_tx_hold_model.py: the
header's five-step rule over the queue models) puts them; ``pending`` and ``deferred`` are the model's; ``busy`` is the
busy model's, the reference's ``__listen`` walked block by block.  Integer outputs and samples: every comparison is
exact."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests import live_tx_hold_model as H
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import capture_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = _native.LIVE_TX_QUEUED
FILL = 0x1234
N, DEPTH, MAXP = 6, 4, 64
PULLS = (2048, 4099, 12288, 12288, 12288)

# kind -> the (baud, training time) of its geometries
KINDS = {"uniform_1200": [(1200, 0.1)],
         "uniform_6000": [(6000, 0.5)],
         "mixed": [(300, 0.02), (1200, 0.1), (6000, 0.5)],        # channel c at entry c % 3
         "rated": [(300, 0.02), (1200, 0.1), (2400, 0.05)]}       # message m of channel c at entry (c + m) % 3


class Station:
    """One transmitter of a kind and its model -- ``HoldTxRatedModel`` for all four: a one-entry table is the uniform
    transmitter, every message of channel c at entry c % 3 the mixed one."""

    _wavs = {}

    def __init__(self, kind, n=N, depth=DEPTH, maxp=MAXP, model_channels=None):
        self.kind, self.n, self.pairs = kind, n, KINDS[kind]
        self.tr = [afskmodem.Transmitter(b, t) for b, t in self.pairs]
        geom = [(48000 // b, t.ts_cycles) for (b, _), t in zip(self.pairs, self.tr)]
        kw = dict(queue_depth=depth, max_payload_len=maxp, device=DEV)
        if kind == "rated":
            self.tx = LiveTransmitter(n, rates=self.tr, **kw)
        elif kind == "mixed":
            self.tx = LiveTransmitter(n, [self.pairs[c % 3][0] for c in range(n)],
                                      [self.pairs[c % 3][1] for c in range(n)], **kw)
        else:
            self.tx = LiveTransmitter(n, self.pairs[0][0], self.pairs[0][1], **kw)
        # model_channels: the transmitter channels the model follows (None: all), for the large transmitters
        self.rows = list(range(n)) if model_channels is None else [int(c) for c in model_channels]
        self.row_of = {c: r for r, c in enumerate(self.rows)}
        self.model = H.HoldTxRatedModel(len(self.rows), geom, depth, maxp, wav=self.wav)
        self.count = {}

    def wav(self, payload, entry):
        key = (self.pairs[entry], payload)
        if key not in Station._wavs:
            Station._wavs[key] = self.tr[entry].wav_samples(payload)
        return Station._wavs[key]

    def entry(self, c):
        m = self.count.get(c, 0)
        self.count[c] = m + 1
        return {"mixed": c % 3, "rated": (c + m) % 3}.get(self.kind, 0)

    def submit(self, chans, pays):
        """Queue on both (chans ascending); returns the model's (status, start, n_samples), checked against the
        transmitter's."""
        entries = [self.entry(c) for c in chans]
        want = self.model.submit([self.row_of[c] for c in chans], pays, entries)
        kw = dict(baud_rate=[self.pairs[e][0] for e in entries]) if self.kind == "rated" else {}
        got = self.tx.submit(chans, pays, **kw).cpu()
        for g, w, name in zip(got, want, ("status", "start", "n_samples")):
            assert (g == w).all(), (name, g.tolist(), w.tolist())
        return want

    def pull(self, torch, T, tag, lens=None, hold=None, holdoff=0, as_tensor=True):
        """One hold pull on both into a buffer of FILL; every sample, pending and deferred compared.  Returns the
        model's deferred."""
        n = self.n
        full = lambda v: v if v is None or len(v) == n else [v[self.row_of[c]] if c in self.row_of else 0  # noqa: E731
                                                             for c in range(n)]
        d_hold = None if hold is None else torch.tensor(full(hold), dtype=torch.int32, device=DEV) if as_tensor \
            else [bool(h) for h in full(hold)]
        d_lens = None if lens is None else torch.tensor(full(lens), dtype=torch.int32, device=DEV)
        out = torch.full((n, T), FILL, dtype=torch.int16, device=DEV)
        got = self.tx.pull(T, out=out, lengths=d_lens, hold=False if d_hold is None else d_hold, holdoff=holdoff)
        m_hold = None if hold is None else [hold[c] if len(hold) == n else hold[self.row_of[c]] for c in self.rows]
        m_lens = None if lens is None else [lens[c] if len(lens) == n else lens[self.row_of[c]] for c in self.rows]
        exp, pend, dfr = self.model.pull_hold(T, m_lens, m_hold, holdoff, FILL)
        idx = torch.tensor(self.rows, device=DEV)
        assert_rows(got[idx].cpu().numpy(), exp, tag)
        assert (self.tx.pending[idx].cpu().numpy() == pend).all(), (tag, "pending")
        assert self.tx.deferred.dtype == torch.int64
        assert (self.tx.deferred[idx].cpu().numpy() == dfr).all(), (tag, "deferred", self.tx.deferred[idx].tolist(),
                                                                    dfr.tolist())
        return dfr, got

    def close(self, torch):
        torch.cuda.synchronize()
        self.tx.close()


def assert_rows(got, exp, tag):
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        c = int(bad[0])
        at = np.nonzero(got[c] != exp[c])[0]
        raise AssertionError((tag, "channels", bad[:5].tolist(), "first column", int(at[0]), "of", at.size,
                              got[c, at[:4]].tolist(), exp[c, at[:4]].tolist()))


def payloads(rng, k, lo=1, hi=8):
    return [bytes(rng.integers(0, 256, int(rng.integers(lo, hi + 1)), dtype=np.uint8)) for _ in range(k)]


def drain(torch, st, tag, limit=40):
    """Unheld 12288-sample pulls until every queue is empty."""
    k = 0
    while st.model.pending().any():
        st.pull(torch, 12288, (tag, "drain", k))
        k += 1
        assert k < limit
    return k


# ------------------------------------------------------------------------------------------------------ 1. holds

@pytest.mark.parametrize("kind", list(KINDS))
def test_holds(torch_cuda, kind):
    """Channel 0: empty and held.  1: a message on an idle channel (start == pos), held in the first pull.  2: two
    messages, held from the second pull on for three pulls -- mid-message, the successor would begin inside one of
    them (0 < delta < L).  3: two messages, held in the second pull alone, while the successor lies wholly beyond it
    (deferred 0).  4: an idle channel's message held over three pulls, then released.  5: never held."""
    torch = torch_cuda
    rng = np.random.default_rng(7)
    st = Station(kind)
    assert st.tx.deferred.shape == (N,) and st.tx.deferred.device == st.tx.pending.device
    deferred_at = st.tx.deferred.data_ptr()
    st.submit([1, 2, 2, 3, 3, 4, 5, 5], payloads(rng, 8, 6, 8))
    holds = [[1, 1, 0, 0, 1, 0], [1, 0, 1, 1, 1, 0], [0, 0, 1, 0, 1, 0], [1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    log = []
    for k, (T, hold) in enumerate(zip(PULLS, holds)):
        before = [list(q) for q in st.model.queue]
        pos = list(st.model.pos)
        dfr, _ = st.pull(torch, T, (kind, k), hold=hold, as_tensor=k != 3)     # (once as a host sequence)
        log.append((T, hold, before, pos, dfr))
    assert st.tx.deferred.data_ptr() == deferred_at                            # a fixed address, like pending
    # what the pattern was built to cover, read from the model
    T0, _, _, _, d0 = log[0]
    assert d0.tolist() == [0, T0, 0, 0, T0, 0]                                 # empty; start == pos; free channels
    assert any(0 < d[2] < T for T, _, _, _, d in log[1:4]), "no successor began inside a held pull"
    T1, _, before, pos, d1 = log[1]
    assert d1[3] == 0 and len(before[3]) == 2 and before[3][1][0] >= pos[3] + T1   # unstarted, wholly beyond the pull
    assert [d[4] for *_, d in log[:4]] == [PULLS[0], PULLS[1], PULLS[2], 0]    # held three pulls, then released
    assert not any(d[5] for *_, d in log) and not any(d[0] for *_, d in log)
    assert drain(torch, st, kind) > 0
    assert not st.tx.pending.any().item()
    st.close(torch)


# ---------------------------------------------------------------------------------------------------- 2. holdoff

@pytest.mark.parametrize("holdoff", [0, 1, 4097, 4099, 30000])
@pytest.mark.parametrize("kind", list(KINDS))
def test_holdoff(torch_cuda, kind, holdoff):
    """4097: an odd start inside a tile; 4099: the wait of channel 0 ends exactly where the second pull ends; 30000:
    a wait that spans several pulls.  Channel 0 is held in the first pull, 1 in the first two, 2 never, 3 is
    mid-message when it is held in the second pull, 4 is empty, 5 is held again in the fourth pull, inside its wait."""
    torch = torch_cuda
    rng = np.random.default_rng(holdoff)
    st = Station(kind)
    st.submit([0, 1, 2, 3, 3, 5], payloads(rng, 6, 6, 8))
    holds = [[1, 1, 0, 0, 1, 1], [0, 1, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0]]
    starts = []
    for k, (T, hold) in enumerate(zip(PULLS, holds)):
        st.pull(torch, T, (kind, holdoff, k), hold=hold, holdoff=holdoff)
        starts.append([q[0][0] if q else None for q in st.model.queue])
    # channel 0 was released after the first pull: its message begins `holdoff` samples behind it
    if holdoff <= PULLS[1]:
        assert starts[1][0] == PULLS[0] + holdoff
    if holdoff == 4099:
        assert st.model.wait[0] == 0 and starts[1][0] == PULLS[0] + PULLS[1]   # exactly at the pull boundary
    if holdoff == 30000:
        assert starts[4][0] == PULLS[0] + 30000 and starts[4][1] == PULLS[0] + PULLS[1] + 30000
    drain(torch, st, (kind, holdoff))
    st.close(torch)


# ------------------------------------------------------------------------------------------------ 3. ragged pulls

@pytest.mark.parametrize("kind", list(KINDS))
def test_ragged_hold_pulls(torch_cuda, kind):
    """Lengths 0, 1, an odd value and T, rotating over the channels, with and without hold: columns at or past
    lengths[c] keep FILL (Station.pull compares the whole buffer), a held channel with length 0 shifts nothing and sets
    its wait."""
    torch = torch_cuda
    rng = np.random.default_rng(3)
    st = Station(kind)
    st.submit([0, 0, 1, 1, 2, 3, 3, 4, 5], payloads(rng, 9, 4, 8))
    pattern = lambda T: (0, 1, T - 1 if T % 2 == 0 else T - 2, T, T + 5, -3)  # noqa: E731
    seen_zero_held = False
    for k, T in enumerate(PULLS + (12288,) * 3):
        lens = [pattern(T)[(c + k) % 6] for c in range(N)]
        hold = [int((c + 2 * k) % 3 == 0) for c in range(N)]
        wait = list(st.model.wait)
        queue = [list(q) for q in st.model.queue]
        dfr, _ = st.pull(torch, T, (kind, k), lens=lens, hold=hold, holdoff=1000 + k)
        for c in range(N):
            if hold[c] and lens[c] <= 0:
                seen_zero_held = True
                assert dfr[c] == 0 and st.model.wait[c] == 1000 + k and list(st.model.queue[c]) == queue[c], (k, c, wait)
    assert seen_zero_held
    drain(torch, st, kind)
    st.close(torch)


# --------------------------------------------------------------------------------------------------- 4. ring paths

@pytest.mark.parametrize("kind", list(KINDS))
def test_a_ring_read_from_global_memory_shifts_four_queued_messages(torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(65)
    st = Station(kind, depth=65)                                # above the 64 entries the tile kernel keeps in LDS
    st.submit([1] * 5 + [4] * 5, payloads(rng, 10, 2, 4))
    st.pull(torch, 2048, (kind, "first"))                       # the first message of each is on air
    before = list(st.model.queue[1])
    # (40960 samples: past the end of the message on air at every rate here, so the four behind it are deferred)
    dfr, _ = st.pull(torch, 40960, (kind, "held"), hold=[0, 1, 0, 0, 0, 0], holdoff=4097)
    after = list(st.model.queue[1])
    moved = [(a[0] - b[0]) for a, b in zip(after[-4:], before[-4:])]
    assert dfr[1] > 0 and moved == [int(dfr[1])] * 4 and dfr[4] == 0
    drain(torch, st, kind, limit=80)
    st.close(torch)


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_wrapped_ring_is_shifted_across_the_wrap(torch_cuda, kind):
    """queue_depth 4: three messages, two retired (head = 2), three more (ring entries 3, 0, 1): the held pull moves
    the entries 3, 0 and 1 while the message in entry 2 is on air."""
    torch = torch_cuda
    rng = np.random.default_rng(4)
    st = Station(kind)
    st.submit([2, 2, 2], payloads(rng, 3, 1, 2))
    k = 0
    while st.model.pending()[2] > 1 or st.model.queue[2][0][0] >= st.model.pos[2]:
        st.pull(torch, 2048, (kind, "retire", k))               # until the third message alone is left, and on air
        k += 1
        assert k < 100
    want = st.submit([2, 2, 2], payloads(rng, 3, 1, 2))
    assert (want[0] == Q).all() and st.model.pending()[2] == 4  # head + count = 2 + 4 > depth
    before = list(st.model.queue[2])
    # (40960 samples: past the end of the message on air at every rate here, so the first waiting one is deferred)
    dfr, _ = st.pull(torch, 40960, (kind, "held"), hold=[0, 0, 1, 0, 0, 0], holdoff=1)
    after = list(st.model.queue[2])
    assert dfr[2] > 0 and len(after) >= 3
    assert [a[0] - b[0] for a, b in zip(after[-3:], before[-3:])] == [int(dfr[2])] * 3
    want = st.submit([2], payloads(rng, 1))                     # (the first has retired: one entry is free)
    assert want[0].tolist() == [Q] and want[1][0] == after[-1][0] + after[-1][1]
    drain(torch, st, kind)
    st.close(torch)


# ---------------------------------------------------------------------------------------------- 5. tiles per block

@pytest.mark.parametrize("n", [4096, 8192], ids=["2_tiles_per_block", "4_tiles_per_block"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_several_tiles_per_block(torch_cuda, kind, n):
    """T = 16384 is four tiles; with 4096 channels a block renders two of them, with 8192 all four.  64 seeded channels
    in neighbouring pairs, one of a pair held and one free; every other channel is silent.  The held ones start 4097
    samples -- an odd offset inside the second tile -- into the second pull, the free ones are held there, mid-message,
    so that their successors move."""
    torch = torch_cuda
    T = 16384
    rng = np.random.default_rng(n)
    first = np.sort(rng.choice(np.arange(0, n - 1, 2), 32, replace=False))
    seeded = np.sort(np.concatenate([first, first + 1]))
    seeded[0], seeded[1], seeded[-2], seeded[-1] = 0, 1, n - 2, n - 1
    seeded = np.unique(seeded)
    st = Station(kind, n=n, depth=4, maxp=8, model_channels=seeded)
    chans = [int(c) for c in seeded for _ in range(3)]
    st.submit(chans, payloads(rng, len(chans), 1, 3))
    odd = [int(c) & 1 for c in seeded]
    even = [1 - h for h in odd]
    idx = torch.from_numpy(seeded).to(DEV)
    moved = 0
    for k, (hold, holdoff) in enumerate(((odd, 4097), (even, 0), (None, 0), (None, 0))):
        dfr, got = st.pull(torch, T, (kind, n, k), hold=hold, holdoff=holdoff)
        assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[idx])), (n, k)   # every other row: silent
        assert not st.tx.deferred.sum().item() - int(dfr.sum())                             # ... and not deferred
        moved += int((dfr > 0).sum())
        if k == 0:
            assert (dfr == np.asarray(odd) * T).all()
        if k == 1:
            assert (dfr[np.asarray(odd) == 1] == 4097).all()    # released: the wait is served inside this pull
    assert moved > len(seeded) // 2
    st.close(torch)


# ------------------------------------------------------------------------------------------ 6. plain-pull equality

@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_hold_all_zero_and_no_holdoff_is_the_plain_pull_bit_for_bit(torch_cuda, kind, ragged):
    torch = torch_cuda
    rng = np.random.default_rng(11)
    a, b = Station(kind), Station(kind)
    chans, pays = [0, 0, 0, 1, 2, 2, 4, 5, 5], payloads(rng, 9, 0, 8)
    a.submit(chans, pays)
    b.submit(chans, pays)
    zero = torch.zeros(N, dtype=torch.int32, device=DEV)
    sound = 0
    for k, T in enumerate(PULLS + (12288,) * 4):
        lens = [(0, 1, T - 1, T)[(c + k) % 4] for c in range(N)] if ragged else None
        oa = torch.full((N, T), FILL, dtype=torch.int16, device=DEV)
        ob = oa.clone()
        hold = (zero, False, [0] * N)[k % 3]
        a.tx.pull(T, out=oa, lengths=lens, hold=hold, holdoff=0)
        b.tx.pull(T, out=ob, lengths=lens)
        assert torch.equal(oa, ob), (kind, k)
        assert torch.equal(a.tx.pending, b.tx.pending) and not a.tx.deferred.any().item(), (kind, k)
        a.tx.deferred.fill_(-1)                                 # (every hold pull writes all of it)
        sound += int(torch.count_nonzero((ob != FILL) & (ob != 0)))
    assert sound > 0
    a.close(torch)
    b.close(torch)


# ---------------------------------------------------------------------------------------------------- 7. state rules

@pytest.mark.parametrize("kind", list(KINDS))
def test_state_rules(torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(2)
    st = Station(kind)
    st.submit([0, 1, 2], payloads(rng, 3, 2, 4))
    st.pull(torch, 4099, (kind, "hold"), hold=[1, 1, 1, 1, 0, 0], holdoff=20000)
    # a submit after a deferral queues behind the shifted end (Station.submit compares the starts)
    want = st.submit([0, 3], payloads(rng, 2, 2, 4))
    assert want[1][0] == st.model.queue[0][0][0] + st.model.queue[0][0][1] and want[1][0] > 4099
    assert want[1][1] == 4099                                   # channel 3: idle, at pos; its wait moves it later
    # a plain and a ragged pull in between neither read nor write the wait: everything due plays, w stays 20000
    out = st.tx.pull(2048).cpu().numpy()
    exp = st.model.expected(2048)
    assert_rows(out, exp, (kind, "plain"))
    assert exp[0].any() and exp[3].any()                        # (channel 0 and 3 are inside their wait, and play)
    assert (st.tx.pending.cpu().numpy() == st.model.pull_ragged(2048, [2048] * N)).all()
    lens = [5, 0, 2048, 77, 1, 0]
    out = torch.full((N, 2048), FILL, dtype=torch.int16, device=DEV)
    st.tx.pull(2048, out=out, lengths=lens)
    assert_rows(out.cpu().numpy(), st.model.expected_ragged(2048, lens, FILL), (kind, "ragged"))
    st.model.pull_ragged(2048, lens)
    assert st.model.wait == [20000, 20000, 20000, 20000, 0, 0]
    # reset(mask) clears the wait of the masked channels only: 1 restarts at once, 2 still waits
    mask = [False, True, False, False, False, True]
    st.tx.reset(mask)
    st.model.reset(mask)
    assert st.model.wait == [20000, 0, 20000, 20000, 0, 0]
    want = st.submit([1, 2, 5], payloads(rng, 3, 2, 4))
    assert want[1][0] == 0 and want[1][2] == 0
    dfr, _ = st.pull(torch, 4099, (kind, "after reset"), hold=None)
    assert dfr[1] == 0 and dfr[5] == 0 and st.model.wait[2] == 20000 - 4099
    drain(torch, st, kind)
    st.close(torch)


# ------------------------------------------------------------------------------------------------------- 8. busy

T_RX = 6144


def busy_capture(n, seed, bfs):
    """One capture per channel (tests/live_drive.capture_of: messages with quiet gaps, in noise), zero padded to a
    multiple of T_RX."""
    rng = np.random.default_rng(seed)
    caps = [capture_of(rng, int(bfs[c]), payloads(rng, 2, 3, 6), training=0.1) for c in range(n)]
    total = -(-max(c.size for c in caps) // T_RX) * T_RX
    host = np.zeros((n, total), np.int16)
    for c, x in enumerate(caps):
        host[c, : x.size] = x
    return host


RX_KINDS = {
    "stored": dict(bit_frames=40, max_burst_len=65536),
    "streaming": dict(bit_frames=40, max_burst_len=None),
    "progressive": dict(bit_frames=40, max_burst_len=None, progressive=True),
    "auto": dict(bit_frames="auto", max_burst_len=None, candidates=[160, 40, 20]),
    "mixed": dict(bit_frames=[40, 160, 20, 40, 160, 20], max_burst_len=65536),
    "mixed_streaming": dict(bit_frames=[40, 160, 20, 40, 160, 20], max_burst_len=None),
}


@pytest.mark.parametrize("kind", list(RX_KINDS))
def test_busy_after_every_push_is_the_gate_recording(torch_cuda, kind):
    torch = torch_cuda
    kw = dict(RX_KINDS[kind])
    bfs = kw.pop("bit_frames")
    rate = [40, 160, 20, 40, 160, 20] if isinstance(bfs, (list, str)) else [40] * N
    host = busy_capture(N, 31, rate)
    dev = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(N, bfs, max_chunk_len=T_RX, device=DEV, **kw)
    models = [H.BusyModel() for _ in range(N)]
    assert rx.busy().tolist() == [0] * N                        # a new receiver
    out = torch.full((N,), 9, dtype=torch.int32, device=DEV)
    seen = [0, 0]
    rng = np.random.default_rng(5)
    p = 0
    while p < host.shape[1]:
        t = min(int(rng.choice([1000, 2048, 4099, T_RX])), host.shape[1] - p)
        res = rx.push(dev[:, p: p + t])
        want = [m.push(host[c, p: p + t]) for c, m in enumerate(models)]
        got = rx.busy(out=out)
        assert got is out and got.tolist() == want, (kind, p)
        if kind == "progressive":
            assert (res.tap.open_start >= 0).to(torch.int32).tolist() == want, (kind, p)
        for w in want:
            seen[w] += 1
        p += t
    assert min(seen) > 10                                       # both answers, many times
    fresh = rx.busy()
    assert fresh.dtype == torch.int32 and fresh.shape == (N,) and fresh.tolist() == out.tolist()
    rx.flush()
    assert rx.busy().tolist() == [0] * N
    for bad in (torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int32)):
        with pytest.raises((TypeError, ValueError)):
            rx.busy(out=bad)
    with pytest.raises(ValueError):
        rx.busy(out=torch.zeros(N + 1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    rx.close()


@pytest.mark.parametrize("streaming", [False, True], ids=["stored", "streaming"])
def test_busy_with_thresholds_per_channel_ragged_pushes_a_flush_mask_and_a_reset(torch_cuda, streaming):
    torch = torch_cuda
    pairs = [(18000, 14000), (9000, 2500), (25000, 20000)] * 2
    host = busy_capture(N, 77, [40] * N)
    dev = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(N, 40, [a for a, _ in pairs], [b for _, b in pairs],
                      max_burst_len=None if streaming else 65536, max_chunk_len=T_RX, device=DEV)
    models = [H.BusyModel(a, b) for a, b in pairs]
    rng = np.random.default_rng(9)
    pos = [0] * N                                               # every channel reads its own capture at its own pace
    seen = [0, 0]
    flushed_busy = reset_busy = 0
    for k in range(200):
        if min(pos) >= host.shape[1]:
            break
        lens = [min(int(rng.choice([0, 1, 2047, 2048, 4099, T_RX])), host.shape[1] - pos[c]) for c in range(N)]
        chunk = torch.zeros((N, T_RX), dtype=torch.int16, device=DEV)
        for c in range(N):
            chunk[c, : lens[c]] = dev[c, pos[c]: pos[c] + lens[c]]
        before = [m.busy for m in models]
        mask = [bool(before[c]) and k % 7 == 3 and c % 2 == 0 for c in range(N)]       # flush some recording channels
        rx.push(chunk, lengths=lens, flush=mask if any(mask) else False)
        want = [m.push(host[c, pos[c]: pos[c] + lens[c]], flush=mask[c]) for c, m in enumerate(models)]
        flushed_busy += sum(mask)
        for c in range(N):                                      # (a flushed channel's new stream reads on from here)
            pos[c] += lens[c]
        assert rx.busy().tolist() == want, (k, "push")
        if k % 11 == 5 and any(want):
            rmask = [bool(w) and c % 2 == 1 for c, w in enumerate(want)]
            rx.reset(rmask)
            for c in range(N):
                if rmask[c]:
                    models[c].reset()
                    reset_busy += 1
            want = [m.busy for m in models]
            assert rx.busy().tolist() == want, (k, "reset")
        for w in want:
            seen[w] += 1
    assert min(pos) >= host.shape[1] and min(seen) > 10 and flushed_busy > 0 and reset_busy > 0
    torch.cuda.synchronize()
    rx.close()


# --------------------------------------------------------------------------------------------------- 9. scenario

T_S = 8192
HEARD = bytes(range(65, 89))                                    # 24 bytes
LEAD = T_S + 300                                                # the first tick is quiet


def scenario_capture():
    burst = afskmodem.Transmitter(1200, 0.5).wav_samples(HEARD)
    assert burst.size == 40 * (600 + 4 + 336) + 4800 == 42400
    host = np.zeros((4, 16 * T_S), np.int16)
    host[1, LEAD: LEAD + burst.size] = burst
    return host


def scenario_station(torch):
    rx = LiveReceiver(4, 40, max_burst_len=65536, max_chunk_len=T_S, device=DEV)
    st = Station("uniform_1200", n=4)
    return rx, st


def test_scenario_a_waiting_message_defers_to_the_burst_being_heard(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(21)
    host = scenario_capture()
    dev = torch.from_numpy(host).to(DEV)
    rx, st = scenario_station(torch)
    free = Station("uniform_1200", n=4)                         # the same messages, nobody ever held
    others = payloads(rng, 3, 6, 8)
    waiting = payloads(rng, 1, 6, 8)
    st.submit([0, 2, 2], others)
    free.submit([0, 2, 2], others)
    busy = torch.zeros(4, dtype=torch.int32, device=DEV)
    gate = H.BusyModel()
    rows, held_ticks, deferred, busy_log = [], [], [], []
    submitted = None
    for t in range(host.shape[1] // T_S):
        rx.push(dev[:, t * T_S:(t + 1) * T_S])
        assert rx.busy(out=busy) is busy
        b = busy.tolist()
        assert b == [0, gate.push(host[1, t * T_S:(t + 1) * T_S]), 0, 0], t
        busy_log.append(b[1])
        if b[1] and submitted is None:                          # a message arrives while the channel is being heard
            st.submit([1], waiting)
            submitted = t
        dfr, got = st.pull(torch, T_S, ("scenario", t), hold=b, holdoff=4800)
        _, unheld = free.pull(torch, T_S, ("free", t))
        assert torch.equal(got[[0, 2, 3]], unheld[[0, 2, 3]]), t   # the other channels are unaffected
        rows.append(got[1].cpu().numpy())
        if b[1]:
            held_ticks.append(t)
            assert not rows[-1].any(), t                        # all zero in every tick whose busy was 1
        deferred.append(int(dfr[1]))
    assert submitted is not None and len(held_ticks) >= 2 and max(deferred) > 0
    assert held_ticks == list(range(held_ticks[0], held_ticks[-1] + 1))
    released = held_ticks[-1] + 1
    assert busy_log[released] == 0
    stream = np.concatenate(rows)
    wav = st.wav(waiting[0], 0)
    assert wav[0] != 0
    begin = released * T_S + 4800                               # 4800 samples after the first tick that reports busy 0
    assert int(np.nonzero(stream)[0][0]) == begin
    assert (stream[begin: begin + wav.size] == wav).all() and not stream[begin + wav.size:].any()
    assert sum(deferred) == begin - submitted * T_S
    st.close(torch)
    free.close(torch)
    rx.close()


def test_push_busy_relay_and_hold_pull_replay_as_one_graph(torch_cuda):
    """push(events=) -> busy(out=) -> submit_events(out=) -> pull(out=, hold=busy) captured once and replayed over the
    scenario: every tick equals the eager run -- the burst heard on channel 1 is relayed onto channel 1 behind the
    message that waited there."""
    torch = torch_cuda
    rng = np.random.default_rng(22)
    host = scenario_capture()
    dev = torch.from_numpy(host).to(DEV)
    ticks = host.shape[1] // T_S
    others, waiting = payloads(rng, 3, 6, 8), payloads(rng, 1, 6, 8)

    def station():
        rx = LiveReceiver(4, 40, max_burst_len=65536, max_chunk_len=T_S, device=DEV)
        tx = LiveTransmitter(4, 1200, 0.1, queue_depth=DEPTH, max_payload_len=MAXP, device=DEV)
        assert (tx.submit([0, 2, 2], others).cpu()[0] == Q).all()
        return (rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(4 * rx.slots),
                torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros((4, T_S), dtype=torch.int16, device=DEV))

    def snapshot(sub, busy, pulled, tx):
        return tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, busy, pulled, tx.pending,
                                                      tx.deferred))

    rx, tx, res, ev, sub, busy, pulled = station()
    eager = []
    for t in range(ticks):
        rx.push(dev[:, t * T_S:(t + 1) * T_S], out=res, events=ev)
        rx.busy(out=busy)
        tx.submit_events(ev, out=sub)
        tx.pull(T_S, out=pulled, hold=busy, holdoff=4800)
        eager.append(snapshot(sub, busy, pulled, tx))
        if t == 1:
            assert (tx.submit([1], waiting).cpu()[0] == Q).all()
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    assert sum(int(e[3][1]) for e in eager) >= 2 and any(e[6][1] > 0 for e in eager)       # held, deferred
    assert sum(int((e[0] == Q).sum()) for e in eager) == 1                                 # the burst was relayed
    assert any(e[4][1].any() for e in eager)

    rx, tx, res, ev, sub, busy, pulled = station()
    chunk = torch.zeros((4, T_S), dtype=torch.int16, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):             # one linear chain
            rx.push(chunk, out=res, events=ev, stream=side)
            rx.busy(out=busy, stream=side)
            tx.submit_events(ev, out=sub, stream=side)
            tx.pull(T_S, out=pulled, hold=busy, holdoff=4800, stream=side)
    torch.cuda.synchronize()
    names = ("status", "start", "n_samples", "busy", "samples", "pending", "deferred")
    for t in range(ticks):
        chunk.copy_(dev[:, t * T_S:(t + 1) * T_S])
        graph.replay()
        for g, w, name in zip(snapshot(sub, busy, pulled, tx), eager[t], names):
            assert (g == w).all(), (t, name)
        if t == 1:
            assert (tx.submit([1], waiting).cpu()[0] == Q).all()
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# ---------------------------------------------------------------------------------------------------- 10. refusals

def test_a_wrong_hold_raises_before_anything_is_launched(torch_cuda):
    torch = torch_cuda
    tx = LiveTransmitter(N, 1200, 0.0, queue_depth=2, max_payload_len=4, device=DEV)
    tx.submit([0], [b"ab"])
    for bad in (torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.bool, device=DEV),
                torch.zeros(N + 1, dtype=torch.int32, device=DEV), torch.zeros((N, 1), dtype=torch.int32, device=DEV),
                [0] * (N - 1), np.zeros(N, np.float32)):
        with pytest.raises(ValueError):
            tx.pull(64, hold=bad)
    with pytest.raises(ValueError):
        tx.pull(64, holdoff=1)
    with pytest.raises(ValueError):
        tx.pull(64, hold=False, holdoff=_native.MAX_STREAM_LEN + 1)
    out = tx.pull(64, hold=True).cpu().numpy()                  # nothing above advanced the channel or set a wait
    assert not out.any() and tx.deferred.tolist() == [64, 0, 0, 0, 0, 0] and tx.pending.tolist() == [1] + [0] * 5
    torch.cuda.synchronize()
    tx.close()
