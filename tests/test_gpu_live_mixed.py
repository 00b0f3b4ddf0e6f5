"""GPU parity (-m gpu) of the live objects with a rate per channel (afsk_live_create_mixed, afsk_live_tx_create_mixed):
interleaved rates must give every channel exactly what a one-rate object of its rate gives it.  The transmitter against
the queue model (tests/live_tx_model.py) fed with ``Transmitter(baud, training_time).wav_samples``, the receiver
against one-rate receivers over the rows of each rate and against ``Receiver.decode_captures``; rate arrays of one
value against the scalar constructors, a graph-captured loopback, and reset.  Expected values never come from a mixed
object itself."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, synth
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import FIELDS, push_sizes, random_payload
from tests.live_tx_model import LiveTxModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = [0, 1, 5, 2047, 2048, 2049, 4000, 8192]              # what a "ragged" chunking draws its push sizes from


class MixedTxModel:
    """One LiveTxModel per channel, each at its channel's geometry, with Transmitter(baud, tt).wav_samples."""

    def __init__(self, bauds, times, depth, mp):
        caches = {}

        def wav_for(baud, tt):
            tr = afskmodem.Transmitter(baud, tt)
            cache = caches.setdefault((baud, tt), {})

            def wav(p):
                if p not in cache:
                    cache[p] = tr.wav_samples(p)
                return cache[p]
            return wav

        self.models = [LiveTxModel(1, 48000 // b, afskmodem.Transmitter(b, t).ts_cycles, depth, mp, wav=wav_for(b, t))
                       for b, t in zip(bauds, times)]

    def submit(self, chans, pays):
        m = len(pays)
        out = [np.zeros(m, np.int32), np.full(m, -1, np.int64), np.zeros(m, np.int32)]
        for i in np.argsort(np.asarray(chans), kind="stable").tolist():
            r = self.models[int(chans[i])].submit([0], [pays[i]])
            for o, v in zip(out, r):
                o[i] = v[0]
        return out

    def expected(self, T):
        return np.concatenate([m.expected(T) for m in self.models])

    def pull(self, T):
        return np.concatenate([m.pull(T) for m in self.models])

    def reset(self, mask):
        for c, m in enumerate(self.models):
            if mask[c]:
                m.reset()


# bit_frames 4, 20, 40, 160 and 2000: small q (4: q = 1; 20: q = 5, an odd quarter symbol), large q (160, 2000), and
# the tiles' data-symbol windows at both ends of the range
TX_BAUDS = (12000, 2400, 1200, 300, 24)


@pytest.mark.parametrize("n", [40, 2048])
def test_mixed_transmitter_against_the_model(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(101 + n)
    depth, mp = 3, 8
    bauds = [TX_BAUDS[i] for i in rng.permutation(np.arange(n) % len(TX_BAUDS))]
    times = [float(rng.choice([0.0, 0.05, 0.1, 0.25])) for _ in range(n)]
    tx = LiveTransmitter(n, bauds, times, queue_depth=depth, max_payload_len=mp, device=DEV)
    assert tx.bit_frames is None and tx.channel_bit_frames.tolist() == [48000 // b for b in bauds]
    model = MixedTxModel(bauds, times, depth, mp)
    odd_idle = 0
    for rnd in range(12):
        k = int(rng.integers(0, 2 * n))
        chans = rng.integers(0, n, k)
        pays = [random_payload(rng, 0, mp) for _ in range(k)]
        idle = [c for c in range(n) if not model.models[c].queue[0] and model.models[c].pos[0] % 2 == 1]
        odd_idle += len(set(idle) & set(chans.tolist()))
        res = tx.submit(chans, pays)
        want = model.submit(chans, pays)
        for g, w, name in zip(res.cpu(), want, ("status", "start", "n_samples")):
            assert (g == w).all(), (rnd, name, np.nonzero(g != w)[0][:5])
        # odd and even T, below and above one 4096-sample tile (and several tiles per block)
        for T in rng.choice([1, 7, 2048, 4095, 4096, 4097, 5001, 8192, 12345, 30001], int(rng.integers(1, 4))):
            T = int(T)
            out = tx.pull(T)
            exp = model.expected(T)
            pend = model.pull(T)
            bad = np.nonzero((out.cpu().numpy() != exp).any(axis=1))[0]
            assert bad.size == 0, (rnd, T, [(int(c), bauds[c]) for c in bad[:5]])
            assert (tx.pending.cpu().numpy() == pend).all(), rnd
    assert odd_idle > 0                                     # messages queued on idle channels at an odd position
    torch.cuda.synchronize()
    tx.close()


def interleaved_captures(n, rates, total, seed):
    """[n, total] device tensor: channel c a live_channels capture at baud rates[c] (48000 / bit_frames)."""
    import torch
    data = torch.empty((n, total), dtype=torch.int16, device=DEV)
    bursts = [None] * n
    for j, bf in enumerate(sorted(set(rates))):
        idx = [c for c in range(n) if rates[c] == bf]
        s, b = synth.live_channels(len(idx), total, 48000 // bf, seed=seed + j, bursts_per_channel=2,
                                   payload_lens=(4, 8, 12), silent_every=7, device=DEV)
        data[torch.tensor(idx, device=DEV)] = s
        for i, c in enumerate(idx):
            bursts[c] = b[i]
    return data, bursts


def collect(res, got, rows=None):
    """Append the bursts of one push to got[c] (c = rows[i] for the i-th channel of the receiver) as dicts."""
    nc = res.n_closed.cpu().numpy()
    if not nc.any():
        return
    bs, bl, fl = (t.cpu().numpy() for t in (res.burst_start, res.burst_len, res.flags))
    d = res.demod.cpu()
    s = res.slots
    for i in np.nonzero(nc)[0].tolist():
        c = rows[i] if rows is not None else i
        for k in range(int(nc[i])):
            j = i * s + k
            row = dict(channel=c, start=int(bs[i, k]), len=int(bl[i, k]), flags=int(fl[i, k]),
                       bytes=d.bytes[j, : min(int(d.nbytes[j]), d.bytes.shape[1])].tobytes())
            row.update({f: int(getattr(d, f)[j]) for f in FIELDS})
            got[c].append(row)


RX_RATES = (160, 80, 40, 20)          # 300 / 600 / 1200 / 2400 baud


@pytest.mark.parametrize("kind", ["2048", "3001", "8192", "ragged"])
def test_mixed_receiver_equals_one_rate_receivers(torch_cuda, kind):
    torch = torch_cuda
    n, total, T = 96, 120000, 8192
    rng = np.random.default_rng(7)
    rates = [RX_RATES[i] for i in rng.permutation(np.arange(n) % 4)]
    data, bursts = interleaved_captures(n, rates, total, seed=21)
    sizes = push_sizes(kind, total, rng, STEPS)
    rx = LiveReceiver(n, rates, max_chunk_len=T, device=DEV)
    assert rx.bit_frames is None and rx.channel_bit_frames.tolist() == rates
    groups = {bf: [c for c in range(n) if rates[c] == bf] for bf in RX_RATES}
    sub = {bf: LiveReceiver(len(idx), bf, max_chunk_len=T, device=DEV) for bf, idx in groups.items()}
    parts = {bf: data[torch.tensor(idx, device=DEV)].contiguous() for bf, idx in groups.items()}
    have, want = [[] for _ in range(n)], [[] for _ in range(n)]
    pos = 0
    for i, t in enumerate(sizes):
        last = i == len(sizes) - 1
        collect(rx.push(data[:, pos: pos + t], flush=last), have)
        for bf, idx in groups.items():
            collect(sub[bf].push(parts[bf][:, pos: pos + t], flush=last), want, idx)
        pos += t
    assert have == want
    assert sum(map(len, have)) >= n                                 # bursts on (nearly) every channel
    # the payloads are what Receiver.decode_captures makes of the whole capture, at each channel's rate
    host = data.cpu().numpy()
    sent = decoded = 0
    for bf, idx in groups.items():
        dec = afskmodem.Receiver(48000 // bf).decode_captures(list(host[idx]), max_bursts=8)
        for c, d in zip(idx, dec):
            assert [g["bytes"] for g in have[c]] == d, c
            sent += len(bursts[c])
            decoded += sum(p in d for _, p in bursts[c])
    assert decoded >= 0.9 * sent, (decoded, sent)                 # (30 dB: the payloads come through)
    torch.cuda.synchronize()
    for r in (rx, *sub.values()):
        r.close()


def test_rate_arrays_of_one_value_are_the_scalar_objects(torch_cuda):
    torch = torch_cuda
    n, total, T = 64, 96000, 4096
    data, _ = synth.live_channels(n, total, 1200, seed=5, bursts_per_channel=2, silent_every=5, device=DEV)
    a = LiveReceiver(n, 40, max_chunk_len=T, device=DEV)
    b = LiveReceiver(n, [40] * n, max_chunk_len=T, device=DEV)
    assert b.bit_frames == 40 and b.state_bytes == a.state_bytes and b.out_stride == a.out_stride
    for pos in range(0, total, T):
        ra = a.push(data[:, pos: pos + T], flush=pos + T >= total)
        rb = b.push(data[:, pos: pos + T], flush=pos + T >= total)
        for x, y in ((ra.n_closed, rb.n_closed), (ra.burst_start, rb.burst_start), (ra.burst_len, rb.burst_len),
                     (ra.flags, rb.flags), (ra.demod.bytes, rb.demod.bytes)):
            assert torch.equal(x, y)
        for f in FIELDS:
            assert torch.equal(getattr(ra.demod, f), getattr(rb.demod, f))
    rng = np.random.default_rng(3)
    s = LiveTransmitter(n, 300, 0.1, device=DEV)
    m = LiveTransmitter(n, np.full(n, 300), [0.1] * n, device=DEV)
    assert (m.baud_rate, m.bit_frames, m.ts_cycles, m.state_bytes) == (300, 160, s.ts_cycles, s.state_bytes)
    chans = np.repeat(np.arange(n), 2)
    pays = [random_payload(rng, 0, 12) for _ in range(2 * n)]
    for x, y in zip(s.submit(chans, pays).cpu(), m.submit(chans, pays).cpu()):
        assert (x == y).all()
    for T in (4097, 1, 30000, 8192):
        assert torch.equal(s.pull(T), m.pull(T))
    torch.cuda.synchronize()
    for o in (a, b, s, m):
        o.close()


def test_graph_captured_mixed_loopback(torch_cuda):
    """4096 channels over four interleaved rates: tx.pull -> rx.push captured as one graph, replayed per chunk."""
    torch = torch_cuda
    n, chunk, per_channel, mp = 4096, 8192, 2, 12
    rng = np.random.default_rng(29)
    bauds = [(300, 600, 1200, 2400)[i] for i in rng.permutation(np.arange(n) % 4)]
    tx = LiveTransmitter(n, bauds, 0.25, queue_depth=per_channel, max_payload_len=mp, device=DEV)
    rx = LiveReceiver.from_receivers([afskmodem.Receiver(b) for b in bauds], max_chunk_len=chunk, device=DEV)
    assert rx.channel_bit_frames.tolist() == tx.channel_bit_frames.tolist()
    pays = [[random_payload(rng, 0, mp) for _ in range(per_channel)] for _ in range(n)]
    res = tx.submit(np.repeat(np.arange(n), per_channel), [p for row in pays for p in row])
    assert (res.status == _native.LIVE_TX_QUEUED).all().item()
    last_end = int((res.start + res.n_samples.to(torch.int64)).max().item())
    assert last_end == int(tx.message_len([len(p) for row in pays for p in row],
                                          np.repeat(np.arange(n), per_channel)).reshape(n, -1).sum(axis=1).max())
    n_chunks = -(-(last_end + 2 * 2048) // chunk)
    buf = torch.zeros((n, chunk), dtype=torch.int16, device=DEV)
    out = rx.alloc_result()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            tx.pull(chunk, out=buf)
            rx.push(buf, out=out)
    torch.cuda.synchronize()
    got = [[] for _ in range(n)]
    for _ in range(n_chunks):
        graph.replay()
        for c, _, _, data in out.bursts():
            got[c].append(data)
    for c, _, _, data in rx.flush().bursts():
        got[c].append(data)
    assert (tx.pending == 0).all().item()
    assert got == pays
    torch.cuda.synchronize()
    del graph
    tx.close()
    rx.close()


def test_reset_on_mixed_objects(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(13)
    # transmitter: reset(mask) mid-message against the model
    n, depth, mp = 64, 3, 8
    bauds = [TX_BAUDS[i % 4] for i in range(n)]
    tx = LiveTransmitter(n, bauds, 0.1, queue_depth=depth, max_payload_len=mp, device=DEV)
    model = MixedTxModel(bauds, [0.1] * n, depth, mp)
    chans = np.repeat(np.arange(n), 2)
    pays = [random_payload(rng, 1, mp) for _ in range(2 * n)]
    tx.submit(chans, pays)
    model.submit(chans, pays)
    assert (tx.pull(5001).cpu().numpy() == model.expected(5001)).all()
    model.pull(5001)
    mask = rng.random(n) < 0.5
    tx.reset(mask)
    model.reset(mask)
    assert (tx.pending.cpu().numpy() == model.pull(0)).all()
    tx.submit([1, 2, 3], [b"x", b"yz", b""])
    model.submit([1, 2, 3], [b"x", b"yz", b""])
    for T in (4097, 30001, 2):
        assert (tx.pull(T).cpu().numpy() == model.expected(T)).all(), T
        assert (tx.pending.cpu().numpy() == model.pull(T)).all()
    # receiver: reset(mask) between pushes, as one-rate receivers with the same mask over their rows
    nr, total, T = 48, 120000, 8192
    rates = [RX_RATES[i % 4] for i in range(nr)]
    data, _ = interleaved_captures(nr, rates, total, seed=31)
    rx = LiveReceiver(nr, rates, max_chunk_len=T, device=DEV)
    groups = {bf: [c for c in range(nr) if rates[c] == bf] for bf in RX_RATES}
    sub = {bf: LiveReceiver(len(idx), bf, max_chunk_len=T, device=DEV) for bf, idx in groups.items()}
    parts = {bf: data[torch.tensor(idx, device=DEV)].contiguous() for bf, idx in groups.items()}
    rmask = rng.random(nr) < 0.5
    have, want = [[] for _ in range(nr)], [[] for _ in range(nr)]
    for pos in range(0, total, T):
        last = pos + T >= total
        if pos == 5 * T:
            rx.reset(rmask)
            for bf, idx in groups.items():
                sub[bf].reset(rmask[idx])
        collect(rx.push(data[:, pos: pos + T], flush=last), have)
        for bf, idx in groups.items():
            collect(sub[bf].push(parts[bf][:, pos: pos + T], flush=last), want, idx)
    assert have == want and sum(map(len, have)) > 0
    torch.cuda.synchronize()
    for o in (tx, rx, *sub.values()):
        o.close()
