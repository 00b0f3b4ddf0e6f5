"""GPU parity (-m gpu) of the rated live transmitter (``LiveTransmitter(n, rates=[...])``, afsk_live_tx_create_rated,
afsk_live_tx_submit_rated, afsk_live_tx_submit_events_rated, live_tx_tile_kernel_rated).

Expected samples never come from the code under test: they are ``Transmitter(baud, t).wav_samples(payload)`` -- the
host mirror the golden digests pin to the reference -- placed where the queue model (tests/live_tx_rated_model.py)
puts them.  Statuses, starts, sample counts and ``pending`` are the model's.  The relay tests read the rate of every
record from the receiver's own ``bit_frames``, so they do not rest on the detector's accuracy.  Integer outputs and
samples: every comparison is exact."""

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests import live_auto_model as A
from tests import live_tx_rated_model as RM
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, FULL, LONG, BAD, UNSORTED = (_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUE_FULL, _native.LIVE_TX_TOO_LONG,
                                _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED)
SKIPPED, NONE, BAD_RATE = _native.LIVE_TX_SKIPPED, _native.LIVE_TX_NONE, _native.LIVE_TX_BAD_RATE


class Table:
    """A rate table as ``Transmitter`` objects: what ``LiveTransmitter(rates=)`` takes, the model's table and the
    expected samples of a message at an entry."""

    def __init__(self, pairs):
        self.tr = [afskmodem.Transmitter(b, t) for b, t in pairs]
        self.bauds = [b for b, _ in pairs]
        self.bf = [48000 // b for b in self.bauds]
        self.geom = [(bf, t.ts_cycles) for bf, t in zip(self.bf, self.tr)]
        self._cache = {}

    def wav(self, payload, entry):
        if (payload, entry) not in self._cache:
            self._cache[payload, entry] = self.tr[entry].wav_samples(payload)
        return self._cache[payload, entry]

    def model(self, n, depth, maxp):
        return RM.LiveTxRatedModel(n, self.geom, depth, maxp, wav=self.wav)

    def live(self, n, depth, maxp):
        return LiveTransmitter(n, rates=self.tr, queue_depth=depth, max_payload_len=maxp, device=DEV)


def assert_outputs(res, want, tag):
    for g, w, name in zip(res.cpu(), want[:3], ("status", "start", "n_samples")):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        assert (g == w).all(), (tag, name, np.nonzero(g != w)[0][:5], g[g != w][:5], w[g != w][:5])


def assert_rows(got, exp, tag):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        c = int(bad[0])
        at = np.nonzero(got[c] != exp[c])[0]
        raise AssertionError((tag, "channels", bad[:5].tolist(), "first column", int(at[0]), "of", at.size,
                              got[c, at[:4]].tolist(), exp[c, at[:4]].tolist()))


# ------------------------------------------------------------------------------------------ 1. every boundary

# bf 4, 20, 40, 160, 2000 and 40 again without training; queued in the order 4, 2000, 20, 160, 40, 40: the small-q
# tone code (bf 4, 20) follows the large-q one and back on one channel
BOUNDARY = Table([(12000, 0.005), (2400, 0.02), (1200, 0.05), (300, 0.1), (24, 0.25), (1200, 0.0)])
ROTATION = (0, 4, 1, 3, 2, 5)
MAXP = 17
LENGTHS = (0, 1, 16, MAXP)
FILL = 0x1234


def boundary_messages(n=6, per_channel=4):
    rng = np.random.default_rng(41)
    chans, pays, entries = [], [], []
    for c in range(n):
        for m in range(per_channel):
            chans.append(c)
            pays.append(bytes(rng.integers(0, 256, LENGTHS[(c + m) % 4], dtype=np.uint8)))
            entries.append(ROTATION[(c + m) % 6])
    return chans, pays, entries


def pull_sizes():
    yield 2048
    yield 4099                                             # odd: every later tile starts at an odd sample
    while True:
        yield 12288


@pytest.mark.parametrize("ragged", [False, True], ids=["plain", "ragged"])
def test_every_pull_renders_each_message_at_its_own_rate(torch_cuda, ragged):
    torch = torch_cuda
    assert BOUNDARY.geom == [(4, 30), (20, 24), (40, 30), (160, 15), (2000, 3), (40, 0)]
    tx, model = BOUNDARY.live(6, 4, MAXP), BOUNDARY.model(6, 4, MAXP)
    assert tx.rated and tx.rates == (12000, 2400, 1200, 300, 24, 1200) and tx.bit_frames is None
    assert tx.baud_rate is None and tx.ts_cycles is None and not tx.channel_bit_frames.any()
    assert tx.rate_bit_frames.tolist() == BOUNDARY.bf and tx.rate_ts_cycles.tolist() == [g[1] for g in BOUNDARY.geom]
    assert tx.rate_bit_frames.dtype == np.int32 and tx.rate_ts_cycles.dtype == np.int32
    assert tx.state_bytes == afskmodem.live.tx_state_bytes_rated(6, 6, 4, MAXP)
    chans, pays, entries = boundary_messages()
    # (a baud rate names the FIRST entry at that rate, so the second 1200-baud entry is reached by index alone: the
    # messages go through the C entry here, through submit(baud_rate=) in the tests below)
    want = model.submit(chans, pays, entries)
    assert (want[0] == Q).all()
    res = submit_by_index(torch, tx, chans, pays, entries)
    assert_outputs(res, want, "submit")
    for p, e, ns in zip(pays, entries, want[2]):
        assert ns == BOUNDARY.wav(p, e).size
        if e != 5:                                         # (a baud rate names the first entry at that rate)
            assert ns == tx.message_len(len(p), baud_rate=BOUNDARY.bauds[e])
    pattern = lambda T: (0, 1, T - 1, T)  # noqa: E731
    pulls = 0
    for k, T in enumerate(pull_sizes()):
        if not model.pending().any():
            break
        assert k < 400
        if ragged:
            lens = [pattern(T)[(c + k) % 4] for c in range(6)]
            out = torch.full((6, T), FILL, dtype=torch.int16, device=DEV)
            got = tx.pull(T, out=out, lengths=lens).cpu().numpy()
            exp = model.expected_ragged(T, lens, FILL)
            pend = model.pull_ragged(T, lens)
        else:
            got = tx.pull(T).cpu().numpy()
            exp = model.expected(T)
            pend = model.pull(T)
        assert_rows(got, exp, (k, T))
        assert (tx.pending.cpu().numpy() == pend).all(), (k, T)
        pulls += 1
    assert pulls > 40 and not tx.pending.any().item()
    torch.cuda.synchronize()
    tx.close()


def submit_by_index(torch, tx, chans, pays, entries, sort=True):
    """afsk_live_tx_submit_rated with device arrays made here: message i on chans[i] at table entry entries[i] (None:
    a NULL rate_index).  sort: stable by channel first, as the Python layer does, the outputs in the caller's order."""
    n = len(pays)
    order = np.argsort(np.asarray(chans), kind="stable") if sort else np.arange(n)
    lens = np.asarray([len(pays[i]) for i in order], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    d_ch = dev(np.asarray(chans, np.int32)[order])
    d_rate = None if entries is None else dev(np.asarray(entries, np.int32)[order])
    d_off, d_len = dev(offs), dev(lens.astype(np.int32))
    d_pay = dev(np.frombuffer(b"".join(pays[i] for i in order) + b"\0", np.uint8).copy())
    d_idx = dev(order.astype(np.int32))
    res = afskmodem.live.SubmitResult(torch.full((n,), 99, dtype=torch.int32, device=DEV),
                                      torch.full((n,), 99, dtype=torch.int64, device=DEV),
                                      torch.full((n,), 99, dtype=torch.int32, device=DEV))
    _native.check(_native.lib().afsk_live_tx_submit_rated(
        tx.handle, n, d_ch.data_ptr(), None if d_rate is None else d_rate.data_ptr(), d_off.data_ptr(),
        d_len.data_ptr(), d_pay.data_ptr(), d_idx.data_ptr(), res.status.data_ptr(), res.start.data_ptr(),
        res.n_samples.data_ptr(), None))
    torch.cuda.synchronize()
    return res


# ------------------------------------------------------------------------------------------ 2. equivalences

def drain(torch, a, b, sizes=(2048, 4099, 12288, 12288, 12288)):
    for T in sizes:
        assert torch.equal(a.pull(T), b.pull(T)), T
        assert torch.equal(a.pending, b.pending), T


@pytest.mark.parametrize("baud", [1200, 6000])
def test_a_one_entry_table_is_the_uniform_transmitter(torch_cuda, baud):
    torch = torch_cuda
    rng = np.random.default_rng(baud)
    rated = LiveTransmitter(5, rates=[baud], training_time=0.1, queue_depth=3, max_payload_len=12, device=DEV)
    plain = LiveTransmitter(5, baud, 0.1, queue_depth=3, max_payload_len=12, device=DEV)
    chans = [4, 0, 2, 2, 0, 2, 2, 7, 1, 2]
    pays = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in (3, 0, 12, 13, 1, 5, 6, 2, 9, 4)]
    for kw in (dict(baud_rate=baud), dict(), dict(baud_rate=[baud] * 10)):
        got, want = rated.submit(chans, pays, **kw).cpu(), plain.submit(chans, pays).cpu()
        for g, w in zip(got, want):
            assert (g == w).all()
        assert set(want[0].tolist()) == {Q, FULL, LONG, BAD}
        drain(torch, rated, plain)
    assert rated.message_len(7) == plain.message_len(7) == rated.message_len(7, baud_rate=baud)
    torch.cuda.synchronize()
    rated.close()
    plain.close()


def test_an_entry_per_channel_is_the_mixed_transmitter(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    bauds, times = [12000, 1200, 300, 2400], [0.01, 0.1, 0.05, 0.0]
    rated = LiveTransmitter(4, rates=bauds, training_time=times, queue_depth=3, max_payload_len=8, device=DEV)
    mixed = LiveTransmitter(4, bauds, times, queue_depth=3, max_payload_len=8, device=DEV)
    assert mixed.bit_frames is None and rated.rate_ts_cycles.tolist() == mixed.channel_ts_cycles.tolist()
    chans = [c for c in range(4) for _ in range(3)]
    pays = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 9, 12)]
    got = rated.submit(chans, pays, baud_rate=[bauds[c] for c in chans]).cpu()
    want = mixed.submit(chans, pays).cpu()
    for g, w in zip(got, want):
        assert (g == w).all()
    assert (want[0] == Q).all()
    drain(torch, rated, mixed, sizes=(2048, 4099) + (12288,) * 6)
    assert not mixed.pending.any().item()
    torch.cuda.synchronize()
    rated.close()
    mixed.close()


# --------------------------------------------------------------------------------- 3. several tiles per block

TILES = Table([(6000, 0.0), (300, 0.0)])                    # bf 8 (small q) and 160 (large q)


@pytest.mark.parametrize("n", [4096, 8192], ids=["2_tiles_per_block", "4_tiles_per_block"])
def test_a_block_of_several_tiles_crosses_from_one_message_to_the_next(torch_cuda, n):
    """T = 16384 is four tiles; with 4096 channels a block renders two of them, with 8192 all four.  A seeded channel
    plays bf 8, 160, 8 back to back: the first ends inside tile 1, the second inside tile 3 -- a block meets a small-q
    and a large-q message whichever way its tiles are grouped."""
    torch = torch_cuda
    T = 16384
    rng = np.random.default_rng(n)
    seeded = np.sort(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), 62, replace=False)]))
    tx, model = TILES.live(n, 4, 8), TILES.model(64, 4, 8)
    chans, rows, pays, entries = [], [], [], []
    for k, c in enumerate(seeded.tolist()):
        for m, (plen, e) in enumerate(((3 + k % 3, 0), (2, 1), (4, 0), (1, 1))):
            chans.append(c)
            rows.append(k)
            pays.append(bytes(rng.integers(0, 256, plen, dtype=np.uint8)))
            entries.append(e)
    want = model.submit(rows, pays, entries)
    starts = want[1].reshape(64, 4)
    assert (want[0] == Q).all() and (4096 < starts[:, 1]).all() and (starts[:, 1] < 8192).all()
    assert (12288 < starts[:, 2]).all() and (starts[:, 2] < T).all()
    res = tx.submit(chans, pays, baud_rate=[TILES.bauds[e] for e in entries])
    assert_outputs(res, want, n)
    for k in range(2):
        got = tx.pull(T)
        idx = torch.from_numpy(seeded).to(DEV)
        assert_rows(got[idx].cpu().numpy(), model.expected(T), (n, k))
        assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[idx])), (n, k)   # every other row: silent
        pend = model.pull(T)
        assert (tx.pending[idx].cpu().numpy() == pend).all() and int(tx.pending.sum()) == int(pend.sum())
    torch.cuda.synchronize()
    tx.close()


# ------------------------------------------------------------------------------------------ 4. the C statuses

def test_the_c_entry_reports_bad_rates_in_the_stated_order(torch_cuda):
    torch = torch_cuda
    table = Table([(1200, 0.0), (6000, 0.0), (1200, 0.01)])
    tx, model = table.live(2, 1, 2), table.model(2, 1, 2)
    # unsorted beats everything; a bad channel beats too long and a bad rate; too long beats a bad rate; a bad rate
    # (-1, n_rates and beyond) beats a full queue
    chans = [0, 0, 0, 0, 0, 1, 1, 5, 0]
    pays = [b"a", b"abc", b"abc", b"b", b"c", b"a", b"a", b"abc", b"abc"]
    entries = [0, 9, 0, -1, 3, 3, 2, 9, 9]
    want = model.submit(chans, pays, entries, sort=False)
    assert want[0].tolist() == [Q, LONG, LONG, BAD_RATE, BAD_RATE, BAD_RATE, Q, BAD, UNSORTED]
    assert_outputs(submit_by_index(torch, tx, chans, pays, entries, sort=False), want, "order")
    want = model.submit([0, 0, 1], [b"a", b"a", b"a"], [0, 3, -7])      # full queues: the bad rate is named first
    assert want[0].tolist() == [FULL, BAD_RATE, BAD_RATE]
    assert_outputs(submit_by_index(torch, tx, [0, 0, 1], [b"a", b"a", b"a"], [0, 3, -7]), want, "full")
    assert_rows(tx.pull(2500).cpu().numpy(), model.expected(2500), "queued")
    assert model.pull(2500).tolist() == tx.pending.cpu().tolist() == [1, 1]       # the refusals queued nothing
    assert_rows(tx.pull(6500).cpu().numpy(), model.expected(6500), "queued")
    assert not model.pull(6500).any() and not tx.pending.any().item()
    # a NULL rate_index: entry 0 for all; the plain entries on a rated transmitter likewise
    want = model.submit([0, 1], [b"xy", b"z"])
    assert_outputs(submit_by_index(torch, tx, [0, 1], [b"xy", b"z"], None), want, "null")
    assert want[2].tolist() == [40 * (4 + 28) + 4800, 40 * (4 + 14) + 4800]
    assert_rows(tx.pull(7000).cpu().numpy(), model.expected(7000), "null")
    assert not model.pull(7000).any()
    want = model.submit([1, 0], [b"q", b"rs"])
    assert_outputs(tx.submit([1, 0], [b"q", b"rs"]), want, "plain entry")
    assert_rows(tx.pull(7000).cpu().numpy(), model.expected(7000), "plain entry")
    model.pull(7000)
    # the rated entry on a transmitter that is not rated: refused, nothing written
    plain = LiveTransmitter(2, 1200, 0.0, queue_depth=1, max_payload_len=2, device=DEV)
    with pytest.raises(_native.AfskNativeError) as ei:
        submit_by_index(torch, plain, [0], [b"a"], [0])
    assert ei.value.code == _native.E_INVALID_ARG and "afsk_live_tx_create_rated" in str(ei.value)
    with pytest.raises(ValueError):
        plain.submit([0], [b"a"], baud_rate=1200)
    with pytest.raises(ValueError):
        tx.submit([0], [b"a"], baud_rate=2400)
    plain.pull(16)
    assert not plain.pending.any().item()
    torch.cuda.synchronize()
    tx.close()
    plain.close()


# --------------------------------------------------------------------------------- 5. into the auto receiver

CALLING = [(300, 0.5), (1200, 0.5), (2400, 0.5)]


def test_loopback_into_the_auto_receiver_names_every_rate_sent(torch_cuda):
    torch = torch_cuda
    table = Table(CALLING)
    n, T = 6, 8192
    rng = np.random.default_rng(17)
    tx = table.live(n, 3, 16)
    rx = LiveReceiver(n, "auto", candidates=[160, 40, 20], max_burst_len=None, max_chunk_len=T, device=DEV)
    chans = [c for c in range(n) for _ in range(3)]
    entries = [(c + m) % 3 for c in range(n) for m in range(3)]
    pays = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in chans]
    st = tx.submit(chans, pays, baud_rate=[table.bauds[e] for e in entries]).cpu()[0]
    assert (st == Q).all()
    whole = [np.concatenate([table.wav(pays[3 * c + m], entries[3 * c + m]) for m in range(3)]) for c in range(n)]
    total = -(-max(w.size for w in whole) // T) * T + T
    want = np.zeros((n, total), np.int16)
    for c, w in enumerate(whole):
        want[c, : w.size] = w
    buf = torch.zeros((n, total), dtype=torch.int16, device=DEV)
    heard = [[] for _ in range(n)]
    for t in range(total // T):
        chunk = tx.pull(T, out=buf[:, t * T:(t + 1) * T])
        for c, _, _, data, bf in rx.push(chunk, flush=t == total // T - 1).rated_bursts():
            heard[c].append((data, bf))
    assert_rows(buf.cpu().numpy(), want, "stream")
    assert not tx.pending.any().item()
    for c in range(n):
        assert heard[c] == [(pays[3 * c + m], table.bf[entries[3 * c + m]]) for m in range(3)], c
    torch.cuda.synchronize()
    tx.close()
    rx.close()


# -------------------------------------------------------------------------------------- 6. relay at the rate heard

HEARD = [(6000, 0.1), (48, 0.1), (2400, 0.1), (300, 0.1), (1200, 0.1), (500, 0.1)]     # bf as live_auto_model.RATES


def relay_run(torch, table, host, cmap=None, skip=None, T=8192):
    """The capture through an auto receiver tick by tick, every tick's events relayed at the rate heard and pulled;
    every output against the relay model.  Returns the records of all ticks with the rate read for each and their
    statuses."""
    n = host.shape[0]
    total = -(-host.shape[1] // T) * T
    d = torch.zeros((n, total), dtype=torch.int16, device=DEV)
    d[:, : host.shape[1]] = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(n, "auto", max_burst_len=None, max_chunk_len=T, max_payload_len=32, device=DEV)
    tx, model = table.live(n, 4, 24), table.model(n, 4, 24)
    ev = rx.alloc_events()
    out = tx.alloc_submit_result(ev.max_events)
    kw = dict(rate="heard", out=out, **({} if cmap is None else dict(channel_map=cmap)),
              **({} if skip is None else dict(skip_flags=skip)))
    skip_flags = _native.LIVE_OPEN_END if skip is None else skip
    log = []
    t = 0
    while t < total // T or model.pending().any():
        assert t < 400
        chunk = d[:, t * T:(t + 1) * T] if t < total // T else torch.zeros((n, T), dtype=torch.int16, device=DEV)
        res = rx.push(chunk, events=ev, flush=t == total // T - 1)
        tx.submit_events(ev, **kw)
        got = tx.pull(T).cpu().numpy()
        rx_bf = res.bit_frames.cpu().numpy()
        buf = ev.buffer.cpu().numpy()
        want = RM.relay_heard(model, buf, ev.max_events, ev.max_bytes, rx.out_stride, n, rx_bf, cmap, skip_flags)
        assert_outputs(out, want, t)
        assert_rows(got, model.expected(T), t)
        assert (tx.pending.cpu().numpy() == model.pull(T)).all(), t
        recs = ev.records().copy()
        log += [(r, int(rx_bf[r["channel"], r["slot"]]), int(s)) for r, s in zip(recs, want[0][: recs.size])]
        t += 1
    torch.cuda.synchronize()
    tx.close()
    rx.close()
    return log


def test_a_relay_repeats_every_burst_at_the_rate_it_was_heard_at(torch_cuda):
    host, sent = A.rate_cases(A.SEED_RATES)
    table = Table(HEARD)
    assert tuple(table.bf) == A.RATES
    log = relay_run(torch_cuda, table, host)
    assert len(log) == 18 and all(s == Q for _, _, s in log)
    assert {bf for _, bf, _ in log} == set(A.RATES)           # (read from the receiver, compared as a set only)


def test_a_rate_the_table_lacks_a_short_burst_and_a_dropped_channel(torch_cuda):
    host, sent = A.rate_cases(A.SEED_RATES)
    host = np.concatenate([host, np.zeros((6, A.BLOCK), np.int16)], axis=1)
    host = np.concatenate([host, np.zeros((6, -host.shape[1] % 8192), np.int16)], axis=1)
    host[:, -A.BLOCK:] = 30000                                 # one loud block before the flush: a TOO_SHORT burst
    table = Table([p for p in HEARD if p[0] != 500])           # nobody answers at bf 96
    log = relay_run(torch_cuda, table, host, cmap=[1, 0, -1, 3, 4, 5], skip=0)
    by_status = {s: [(int(r["channel"]), bf, int(r["status"])) for r, bf, s2 in log if s2 == s]
                 for s in {s for _, _, s in log}}
    assert set(by_status) == {Q, BAD_RATE, SKIPPED}
    assert by_status[BAD_RATE] and all(bf == 96 and ch != 2 for ch, bf, _ in by_status[BAD_RATE])
    assert all(bf != 96 and bf in table.bf and ch != 2 for ch, bf, _ in by_status[Q])
    short = [x for x in by_status[SKIPPED] if x[2] == _native.ST_TOO_SHORT]
    assert len(short) == 6 and all(bf == 0 for _, bf, _ in short)
    assert all(ch == 2 or st != _native.ST_OK for ch, _, st in by_status[SKIPPED])
    assert any(ch == 2 and st == _native.ST_OK for ch, _, st in by_status[SKIPPED])


def test_push_relay_and_pull_replay_as_one_graph(torch_cuda):
    torch = torch_cuda
    T, n = 16384, 4
    rng = np.random.default_rng(23)
    table = Table([(2400, 0.0), (1200, 0.0)])
    caps = [A.rated_capture(rng, [((20, 40)[c % 2], bytes(rng.integers(0, 256, 4, dtype=np.uint8)))])
            for c in range(n)]
    host = A.stack(caps)
    # every message ends inside the second tick: no burst closes in the first, all have closed after the second
    assert host.shape[1] <= 3 * T
    dev = torch.zeros((n, 3 * T), dtype=torch.int16, device=DEV)
    dev[:, : host.shape[1]] = torch.from_numpy(host).to(DEV)

    def station():
        rx = LiveReceiver(n, "auto", candidates=[20, 40], max_burst_len=None, max_chunk_len=T, device=DEV)
        tx = table.live(n, 2, 8)
        return rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(n * rx.slots)

    rx, tx, res, ev, sub = station()
    eager = []
    for t in range(2):
        rx.push(dev[:, t * T:(t + 1) * T], out=res, events=ev)
        tx.submit_events(ev, out=sub, rate="heard")
        pulled = tx.pull(T)
        eager.append(tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, pulled, tx.pending,
                                                            res.bit_frames)))
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    assert (eager[0][0] == NONE).all() and int((eager[1][0] == Q).sum()) == n and eager[1][3].any()
    assert set(eager[1][2][eager[1][0] == Q].tolist()) <= {20 * (4 + 56) + 4800, 40 * (4 + 56) + 4800}

    rx, tx, res, ev, sub = station()
    chunk = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    pulled = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):             # one linear chain: push, pack, submit, pull
            rx.push(chunk, out=res, events=ev, stream=side)
            tx.submit_events(ev, out=sub, rate="heard", stream=side)
            tx.pull(T, out=pulled, stream=side)
    torch.cuda.synchronize()
    for t in range(2):
        chunk.copy_(dev[:, t * T:(t + 1) * T])
        graph.replay()
        got = tuple(x.cpu().numpy() for x in (sub.status, sub.start, sub.n_samples, pulled, tx.pending,
                                              res.bit_frames))
        for g, w, name in zip(got, eager[t], ("status", "start", "n_samples", "samples", "pending", "bit_frames")):
            assert (g == w).all(), (t, name)
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# ------------------------------------------------------------------------------------------------------ 7. reset

def test_reset_drops_the_half_sent_messages_of_the_masked_channels_only(torch_cuda):
    torch = torch_cuda
    table = Table([(6000, 0.0), (300, 0.02), (1200, 0.01)])
    tx, model = table.live(4, 3, 6), table.model(4, 3, 6)
    chans = [0, 0, 1, 1, 2, 3, 3, 3]
    entries = [1, 0, 0, 1, 2, 2, 1, 0]
    pays = [bytes([65 + i] * (i % 6 + 1)) for i in range(8)]
    bauds = [table.bauds[e] for e in entries]
    assert_outputs(tx.submit(chans, pays, baud_rate=bauds), model.submit(chans, pays, entries), "submit")
    assert_rows(tx.pull(3001).cpu().numpy(), model.expected(3001), "first")    # every first message is half sent
    pend = model.pull(3001)
    assert pend.tolist() == [2, 2, 1, 3] and (tx.pending.cpu().numpy() == pend).all()
    mask = [True, False, True, False]
    tx.reset(mask)
    model.reset(mask)
    assert tx.pending.cpu().tolist() == [0, 2, 0, 3]
    # the reset channels restart at sample 0 with new messages at other rates; the others play on
    again = ([0, 2, 2], [b"new", b"er", b"!"], [2, 0, 1])
    assert_outputs(tx.submit(again[0], again[1], baud_rate=[table.bauds[e] for e in again[2]]),
                   model.submit(*again), "again")
    for k, T in enumerate((4099, 12288, 12288, 12288, 12288)):
        assert_rows(tx.pull(T).cpu().numpy(), model.expected(T), ("after", k))
        assert (tx.pending.cpu().numpy() == model.pull(T)).all(), k
    tx.reset()
    model.reset()
    assert not tx.pending.any().item()
    assert not tx.pull(2048).any().item()
    torch.cuda.synchronize()
    tx.close()
