"""GPU parity (-m gpu) of the live objects over every rate they accept and over their long-running and deep-queue
paths: the transmitter at all 48 rates (uniform and mixed objects), with deep rings, four tiles per wave and stream
positions past 2^31 and 2^32 samples; the receiver at all 36 rates (uniform, mixed at scale, loopback) and past 2^31
and 2^32 samples, with a burst longer than 2^31 samples.  Expected values never come from a live object: the queue
model (tests/live_tx_model.py, fed by ``Transmitter.wav_samples``), the CPU oracle, ``batch.demod_batch`` and
``Receiver.decode_captures`` on the same samples, and the sent payloads."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, synth
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from oracle import afsk_oracle as O
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live import check_demod_against_batch, oracle_bursts
from tests.test_gpu_live_mixed import FIELDS, MixedTxModel, collect

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK = 2048
TILE = 4096
TX_BFS = tuple(bf for bf in range(4, 48001, 4) if 48000 % bf == 0)       # 48 rates: 12000 ... 1 baud
RX_BFS = tuple(bf for bf in range(4, 2048, 4) if 48000 % bf == 0)        # 36 rates: 12000 ... 24 baud
SMALL_PULLS = (0, 1, 7, 4095, 4096, 4097, 8191, 30001)
SMALL_P = (0.08, 0.1, 0.1, 0.1, 0.1, 0.1, 0.12, 0.3)
BIG_PULLS = (1 << 20, (1 << 20) - 1, 777777)


def random_payload(rng, n):
    return bytes(rng.integers(0, 256, int(n), dtype=np.uint8))


def positive_training(baud):
    """A training time with ts_cycles > 0 at this rate."""
    tt = max(0.02, 2.5 / baud)
    assert afskmodem.Transmitter(baud, tt).ts_cycles > 0
    return tt


def tx_budget(bf):
    """Samples one message may take: 3 M from 2400 samples per symbol on (pulls up to 2^20), less below."""
    return 3_000_000 if bf >= 2400 else min(3_000_000, 60_000 + 100 * bf)


def tx_plen_max(bf, ts):
    """The longest payload whose message fits tx_budget(bf), at most 256 bytes (256 from bf 12 down: a data phase of
    at least three tiles)."""
    return int(min(256, max(0, (tx_budget(bf) - 4800) // bf - 4 - 2 * max(ts, 0)) // 14))


def pull_size(rng, big):
    if big and rng.random() < 0.5:
        return int(rng.choice(BIG_PULLS))
    return int(rng.choice(SMALL_PULLS, p=SMALL_P))


def rows_expected(model, rows, T):
    return np.stack([model.models[c].expected(T)[0] for c in rows])


def idle_at_odd(model, c):
    m = model.models[c]
    return not m.queue[0] and m.pos[0] % 2 == 1


def check_pull(tx, model, T, rows=None, tag=None):
    """One pull of T against the model (every row, or `rows`), and pending."""
    out = tx.pull(T)
    if rows is None:
        got, exp = out.cpu().numpy(), model.expected(T)
    else:
        import torch
        got = out[torch.as_tensor(rows, device=DEV)].cpu().numpy()
        exp = rows_expected(model, rows, T)
    pend = model.pull(T)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (tag, T, bad[:5].tolist())
    assert (tx.pending.cpu().numpy() == pend).all(), (tag, T)


def check_submit(tx, model, chans, pays, tag=None):
    res = tx.submit(chans, pays)
    want = model.submit(chans, pays)
    for g, w, name in zip(res.cpu(), want, ("status", "start", "n_samples")):
        assert (g == w).all(), (tag, name, np.nonzero(g != w)[0][:5].tolist())
    return want


def drive_tx(tx, model, rng, plens, big, rounds=3, tag=None):
    """A pull of 7 samples (every channel idle at an odd position), then rounds of submit (round 0: every channel at
    its longest payload; later: a random half, idle channels among them) and one to three pulls; then pulls until every
    queue has drained.  Every submit output and pull against the model.  Returns how many messages were queued on a
    channel that was idle at an odd stream position."""
    n = len(plens)
    check_pull(tx, model, 7, tag=tag)
    odd_idle = 0
    for rnd in range(rounds):
        chans = np.arange(n) if rnd == 0 else np.sort(rng.choice(n, max(1, n // 2), replace=False))
        odd_idle += sum(idle_at_odd(model, int(c)) for c in chans)
        pays = [random_payload(rng, plens[c] if rnd == 0 else rng.integers(0, plens[c] + 1)) for c in chans]
        check_submit(tx, model, chans, pays, tag=(tag, rnd))
        for _ in range(int(rng.integers(1, 4))):
            check_pull(tx, model, pull_size(rng, big), tag=(tag, rnd))
    for _ in range(100000):
        if not model.pull(0).any():
            break
        check_pull(tx, model, pull_size(rng, big), tag=(tag, "drain"))
    assert not tx.pending.cpu().numpy().any()
    return odd_idle


# ------------------------------------------------------------------------------------------------ transmitter
@pytest.mark.parametrize("bf", TX_BFS)
def test_tx_every_rate_uniform(torch_cuda, bf):
    """One uniform object per rate and training (ts_cycles 0 and > 0): q < 8 and q >= 8 tile kernels, symbols longer
    than a tile from bf 4096 on, data phases of three tiles and more at bf <= 12."""
    torch = torch_cuda
    baud = 48000 // bf
    rng = np.random.default_rng(1000 + bf)
    n = 3
    odd_idle = 0
    for tt in (0.0, positive_training(baud)):
        tx = LiveTransmitter(n, baud, tt, queue_depth=3, max_payload_len=256, device=DEV)
        assert tx.bit_frames == bf and (tx.ts_cycles > 0) == (tt > 0)
        model = MixedTxModel([baud] * n, [tt] * n, 3, 256)
        pm = tx_plen_max(bf, tx.ts_cycles)
        plens = [pm, max(pm // 2, 0), max(pm - 1, 0)]
        if bf <= 12:
            assert pm == 256 and bf * 14 * 256 >= 3 * TILE
        odd_idle += drive_tx(tx, model, rng, plens, big=bf >= 2400, tag=(bf, tt))
        torch.cuda.synchronize()
        tx.close()
    assert odd_idle > 0


def test_tx_every_rate_mixed(torch_cuda):
    """One mixed object over all 48 rates, interleaved, with per-channel training times (ts_cycles 0 and > 0)."""
    torch = torch_cuda
    rng = np.random.default_rng(4848)
    n = 2 * len(TX_BFS)
    order = rng.permutation(np.arange(n) % len(TX_BFS))
    bauds = [48000 // TX_BFS[i] for i in order]
    seen, times = set(), []
    for b in bauds:                                          # every rate once without and once with training
        times.append(positive_training(b) if b in seen else 0.0)
        seen.add(b)
    tx = LiveTransmitter(n, bauds, times, queue_depth=3, max_payload_len=256, device=DEV)
    assert tx.bit_frames is None and sorted(set(tx.channel_bit_frames.tolist())) == list(TX_BFS)
    assert (tx.channel_ts_cycles == 0).sum() == len(TX_BFS) and (tx.channel_ts_cycles > 0).sum() == len(TX_BFS)
    model = MixedTxModel(bauds, times, 3, 256)
    plens = [tx_plen_max(int(bf), int(ts)) for bf, ts in zip(tx.channel_bit_frames, tx.channel_ts_cycles)]
    assert drive_tx(tx, model, rng, plens, big=True, tag="mixed") > 0
    torch.cuda.synchronize()
    tx.close()


@pytest.mark.parametrize("depth", [65, 300])
@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_tx_deep_queues(torch_cuda, depth, kind):
    """Rings deeper than the 64 entries read from LDS: many short messages, the head wrapping the ring several times,
    tiles whose scan walks past ring index 64, and submits into a full queue (QUEUE_FULL against the model)."""
    torch = torch_cuda
    rng = np.random.default_rng(depth + (kind == "mixed"))
    n, mp = 8, 2
    bauds = [2400] * n if kind == "uniform" else [(12000, 2400, 1200, 6000)[c % 4] for c in range(n)]
    times = [0.0] * n if kind == "uniform" else [(0.0, 0.01)[c % 2] for c in range(n)]
    tx = LiveTransmitter(n, bauds if kind == "mixed" else 2400, times if kind == "mixed" else 0.0,
                         queue_depth=depth, max_payload_len=mp, device=DEV)
    assert (tx.bit_frames is None) == (kind == "mixed")
    model = MixedTxModel(bauds, times, depth, mp)
    full = queued = 0
    longest = int(tx.message_len(mp, np.arange(n)).max()) if kind == "mixed" else int(tx.message_len(mp))
    for rnd in range(5):
        # refill every queue and overfill it: depth + 7 messages per channel
        k = depth + 7
        chans = np.repeat(np.arange(n), k)
        pays = [random_payload(rng, rng.integers(0, mp + 1)) for _ in chans]
        st, _, _ = check_submit(tx, model, chans, pays, tag=rnd)
        full += int((st == _native.LIVE_TX_QUEUE_FULL).sum())
        queued += int((st == _native.LIVE_TX_QUEUED).sum())
        # one pull over most of the queue (the last tiles scan far into the ring), then a few odd ones
        check_pull(tx, model, min(depth * longest * 3 // 4, (1 << 20) + 3), tag=rnd)
        for _ in range(3):
            check_pull(tx, model, int(rng.choice([1, 4097, 30001, 8191, 131071])), tag=rnd)
    while model.pull(0).any():
        check_pull(tx, model, (1 << 20) - 1, tag="drain")
    assert full >= 5 * 7 * n and queued > 3 * depth * n       # the head went round the ring several times
    torch.cuda.synchronize()
    tx.close()


@pytest.mark.parametrize("kind", ["uniform", "mixed"])
def test_tx_four_tiles_per_wave(torch_cuda, kind):
    """n * ceil(T / 4096) >= 4 * 8192: one wave renders 4 consecutive tiles; 10 tiles per row (3 blocks, the last
    with 2 tiles, the last of them 5 samples long).  A seeded sample of rows against the model."""
    torch = torch_cuda
    rng = np.random.default_rng(44 if kind == "uniform" else 45)
    n, T = 4096, 9 * TILE + 5
    assert n * -(-T // TILE) >= 4 * 8192 and -(-T // TILE) % 4 != 0
    if kind == "uniform":
        bauds, times = [12000] * n, [0.0] * n
    else:
        bauds = [48000 // TX_BFS[i] for i in rng.permutation(np.arange(n) % len(TX_BFS))]
        times = [float(rng.choice([0.0, 0.05])) for _ in range(n)]
    mp = 256
    tx = LiveTransmitter(n, bauds if kind == "mixed" else 12000, times if kind == "mixed" else 0.0, queue_depth=2,
                         max_payload_len=mp, device=DEV)
    model = MixedTxModel(bauds, times, 2, mp)
    rows = np.sort(rng.choice(n, 384, replace=False)).tolist()
    check_pull(tx, model, 3, rows, tag=kind)                 # odd stream positions
    plens = [min(mp, tx_plen_max(48000 // b, 0)) if b >= 2400 else int(rng.integers(0, 3)) for b in bauds]
    chans = np.repeat(np.arange(n), 2)                      # two messages back to back: tones in the last tile
    check_submit(tx, model, chans, [random_payload(rng, plens[c]) for c in chans], tag=kind)
    for k in range(4):
        check_pull(tx, model, T, rows, tag=(kind, k))
    torch.cuda.synchronize()
    tx.close()


def tx_silent_until(torch, tx, model, buf, target):
    """Pull up to stream position `target` in pulls of at most buf's width, all silent: checked on the device (a
    nonzero count), with nothing on air in the model."""
    nz = torch.zeros((), dtype=torch.int64, device=DEV)
    pos = model.models[0].pos[0]
    C = buf.shape[1]
    while pos < target:
        t = min(C, target - pos)
        assert not any(m.on_air[0] for m in model.models)
        nz += torch.count_nonzero(tx.pull(t, out=buf))
        model.pull(t)
        pos += t
    assert nz.item() == 0, target


def test_tx_past_2_31_and_2_32_samples(torch_cuda):
    """int64 stream positions: messages straddling sample 2^31 and 2^32, queued at even and odd positions; their
    submit starts and the pulls around them exactly against the model, the silence between checked on the device."""
    torch = torch_cuda
    bauds, times = [12000, 1200, 300, 2400], [0.1, 0.1, 0.0, 0.25]
    n = len(bauds)
    tx = LiveTransmitter(n, bauds, times, queue_depth=4, max_payload_len=16, device=DEV)
    model = MixedTxModel(bauds, times, 4, 16)
    buf = torch.empty((n, 1 << 24), dtype=torch.int16, device=DEV)
    rng = np.random.default_rng(31)
    for boundary in (1 << 31, 1 << 32):
        tx_silent_until(torch, tx, model, buf, boundary - 3000)
        # channels 0 and 1 queue at an even position, 2 and 3 one sample later (odd)
        starts = []
        st, s, _ = check_submit(tx, model, [0, 1], [b"straddle", b"at 2^31 or 2^32"], tag=boundary)
        starts += s.tolist()
        check_pull(tx, model, 1, tag=boundary)
        st2, s2, _ = check_submit(tx, model, [3, 2], [random_payload(rng, 9), random_payload(rng, 3)], tag=boundary)
        starts += s2.tolist()
        assert (st == 0).all() and (st2 == 0).all()
        assert starts == [boundary - 3000] * 2 + [boundary - 2999] * 2
        for c in range(n):                                   # every message's tones straddle the boundary
            s0, ns, _ = model.models[c].on_air[0][0]
            assert s0 < boundary < s0 + ns - 4800, c
        # a second message behind the first on channel 1 (busy: it follows with no gap)
        check_submit(tx, model, [1], [b"next"], tag=boundary)
        while model.pull(0).any():
            check_pull(tx, model, int(rng.choice([4097, 30001, 8191, 1, 65536])), tag=boundary)
    assert model.models[0].pos[0] > 1 << 32
    torch.cuda.synchronize()
    tx.close()


# ------------------------------------------------------------------------------------------------ receiver
def rx_payload_lens(bf, share=None):
    if share is None:
        return (4, 12, 24) if bf <= 40 else (2, 4, 8) if bf <= 400 else (1, 2)
    ts = synth.ts_cycles_for(48000 // bf, 0.25)
    fit = tuple(p for p in (1, 2, 4, 8, 12) if synth.frames_needed(bf, ts, p) + 5 * BLOCK <= share)
    assert fit, bf
    return fit


def rx_total(bf, bursts=2):
    ts = synth.ts_cycles_for(48000 // bf, 0.25)
    need = synth.frames_needed(bf, ts, max(rx_payload_lens(bf))) + 6 * BLOCK
    return bursts * -(-need // BLOCK) * BLOCK


def ragged_sizes(total, rng, choices, head=(1, 2047, 2049, 1, 2048)):
    """Push sizes summing to total: `head`, then drawn from `choices`."""
    out, left = [], total
    while left > 0:
        t = min(head[len(out)] if len(out) < len(head) else int(rng.choice(choices)), left)
        out.append(t)
        left -= t
    return out


def push_all(rx, data, sizes):
    got = [[] for _ in range(data.shape[0])]
    pos = 0
    for i, t in enumerate(sizes):
        collect(rx.push(data[:, pos: pos + t], flush=i == len(sizes) - 1), got)
        pos += t
    assert pos == data.shape[1]
    return got


@pytest.mark.parametrize("bf", RX_BFS)
def test_rx_every_rate_uniform(torch_cuda, bf):
    """A uniform receiver at each of the 36 rates, ragged pushes (1, 2047, 2049 ...): the bursts equal the oracle's
    gate over the whole capture, every burst's demod equals demod_batch on those samples (and the oracle's load_frames
    of them), and the sent payloads come through at 30 dB."""
    torch = torch_cuda
    baud = 48000 // bf
    rng = np.random.default_rng(bf)
    n, total = 12, rx_total(bf)
    data, bursts = synth.live_channels(n, total, baud, seed=500 + bf, bursts_per_channel=2,
                                       payload_lens=rx_payload_lens(bf), silent_every=7, device=DEV)
    rx = LiveReceiver(n, bf, max_burst_len=1 << 18, max_chunk_len=8192, device=DEV)
    got = push_all(rx, data, ragged_sizes(total, rng, [1, 5, 2047, 2048, 2049, 4000, 8192]))
    host = data.cpu().numpy()
    sent = decoded = 0
    for c in range(n):
        assert [(g["start"], g["len"], g["flags"]) for g in got[c]] == oracle_bursts(host[c], 18000, 14000), c
        for g in got[c]:
            assert g["bytes"] == O.load_frames(host[c, g["start"]: g["start"] + g["len"]], baud, 14000), c
        sent += len(bursts[c])
        decoded += sum(p in [g["bytes"] for g in got[c]] for _, p in bursts[c])
    assert sum(map(len, got)) >= sent
    assert check_demod_against_batch(torch, data, got, bf, 14000, rx.out_stride) == sum(map(len, got))
    if bf in (4, 2000):                                      # the CPU oracle's demod fields as well
        spans = [(c, g) for c in range(n) for g in got[c]]
        want = O.demod_batch(host.reshape(-1), np.array([c * total + g["start"] for c, g in spans], np.int64),
                             np.array([g["len"] for _, g in spans], np.int32), np.full(len(spans), bf, np.int32), 14000,
                             out_stride=rx.out_stride)
        for j, (c, g) in enumerate(spans):
            for f in FIELDS:
                assert g[f] == int(want[f][j]), (c, f)
            assert g["bytes"] == want["bytes"][j, : int(want["nbytes"][j])].tobytes(), c
    # 12000 baud: the reference's .wav quirk destroys the mark tone (ref:239-244), no payload survives it; from
    # 1200 samples per symbol on the reference's clock recovery needs the burst near a block boundary
    if bf == 4:
        assert decoded == 0
    elif bf < 1200:
        assert decoded >= 0.9 * sent, (decoded, sent)
    torch.cuda.synchronize()
    rx.close()


def test_rx_mixed_all_rates_at_scale(torch_cuda):
    """One mixed receiver over all 36 rates, 80 channels per rate, pushes of up to 16384 samples: n * slots >= 8256
    (the plan spans several 4096-slot windows and the large-launch paths).  Field by field against 36 one-rate
    receivers over the same rows; a seeded sample against Receiver.decode_captures."""
    torch = torch_cuda
    per, total, T = 80, 131072, 16384
    n = per * len(RX_BFS)
    rng = np.random.default_rng(3636)
    rates = [RX_BFS[i] for i in rng.permutation(np.arange(n) % len(RX_BFS))]
    data = torch.empty((n, total), dtype=torch.int16, device=DEV)
    groups = {bf: [c for c in range(n) if rates[c] == bf] for bf in RX_BFS}
    for j, (bf, idx) in enumerate(groups.items()):
        s, _ = synth.live_channels(len(idx), total, 48000 // bf, seed=900 + j, bursts_per_channel=2,
                                   payload_lens=rx_payload_lens(bf, total // 2), silent_every=7, device=DEV)
        data[torch.tensor(idx, device=DEV)] = s
        del s
    rx = LiveReceiver(n, rates, max_burst_len=65536, max_chunk_len=T, device=DEV)
    assert rx.bit_frames is None and n * rx.slots >= 8256
    sub = {bf: LiveReceiver(len(idx), bf, max_burst_len=65536, max_chunk_len=T, device=DEV)
           for bf, idx in groups.items()}
    parts = {bf: data[torch.tensor(idx, device=DEV)].contiguous() for bf, idx in groups.items()}
    have, want = [[] for _ in range(n)], [[] for _ in range(n)]
    pos = 0
    sizes = ragged_sizes(total, rng, [2047, 2049, 8192, 12345, 16384], head=(1, 2047, 2049))
    for i, t in enumerate(sizes):
        last = i == len(sizes) - 1
        collect(rx.push(data[:, pos: pos + t], flush=last), have)
        for bf, idx in groups.items():
            collect(sub[bf].push(parts[bf][:, pos: pos + t], flush=last), want, idx)
        pos += t
    assert have == want
    assert sum(map(len, have)) >= n
    sample = {bf: rng.choice(idx, 3, replace=False).tolist() for bf, idx in groups.items()}
    for bf, idx in sample.items():
        host = data[torch.tensor(idx, device=DEV)].cpu().numpy()
        dec = afskmodem.Receiver(48000 // bf).decode_captures(list(host), max_bursts=8)
        assert [[g["bytes"] for g in have[c]] for c in idx] == dec, bf
    torch.cuda.synchronize()
    for r in (rx, *sub.values()):
        r.close()


def test_rx_loopback_all_rates(torch_cuda):
    """A mixed LiveTransmitter feeds a mixed LiveReceiver over all 36 shared rates on clean signal, chunk by chunk.
    Each message is queued when its channel is idle at a chunk boundary (a block boundary, where the reference's clock
    recovery holds at every rate); every payload comes back in order -- at 12000 baud, where the reference's .wav quirk
    destroys the mark tone, what Receiver.decode_captures makes of the same samples."""
    torch = torch_cuda
    rng = np.random.default_rng(7272)
    n, chunk, per_channel = 2 * len(RX_BFS), 8192, 2
    bauds = [48000 // RX_BFS[i] for i in rng.permutation(np.arange(n) % len(RX_BFS))]
    tx = LiveTransmitter(n, bauds, 0.25, queue_depth=per_channel, max_payload_len=8, device=DEV)
    rx = LiveReceiver(n, [48000 // b for b in bauds], max_burst_len=1 << 18, max_chunk_len=chunk, device=DEV)
    pays = [[random_payload(rng, rng.integers(1, (8 if b >= 300 else 2) + 1)) for _ in range(per_channel)]
            for b in bauds]
    left = [list(p) for p in pays]
    got = [[] for _ in range(n)]
    captured = []
    busy_until = np.zeros(n, np.int64)
    pos = 0
    for _ in range(100000):
        # (not at sample 0: the gate discards a stream's first block; after a message two more blocks, for the
        # block that closes its burst and the one discarded after it)
        idle = [c for c in range(n) if left[c] and busy_until[c] + 2 * BLOCK <= pos]
        if idle and pos > 0:
            st, s, ns = tx.submit(idle, [left[c].pop(0) for c in idle]).cpu()
            assert (st == _native.LIVE_TX_QUEUED).all() and (s == pos).all()
            busy_until[idle] = s + ns
        if not any(left) and busy_until.max() + 2 * BLOCK <= pos:
            break
        win = tx.pull(chunk)
        captured.append(win.cpu().numpy())
        for c, _, _, data in rx.push(win).bursts():
            got[c].append(data)
        pos += chunk
    for c, _, _, data in rx.flush().bursts():
        got[c].append(data)
    assert (tx.pending == 0).all().item()
    host = np.concatenate(captured, axis=1)
    for c in range(n):
        if bauds[c] == 12000:
            assert got[c] == afskmodem.Receiver(12000).decode_captures([host[c]], max_bursts=8)[0], c
        else:
            assert got[c] == pays[c], (c, bauds[c])
    torch.cuda.synchronize()
    tx.close()
    rx.close()


def test_rx_past_2_31_and_2_32_samples(torch_cuda):
    """int64 stream positions in the receiver.  Channel 0: silence, then bursts straddling sample 2^31, starting past
    it, and straddling 2^32 (pushed from odd stream positions, with ragged pushes); their starts equal the oracle's
    gate offsets plus the samples already pushed, their demod the oracle's.  Channel 1: a loud signal for more than
    2^31 samples -- reported with burst_len 2^31 - 2048 and LIVE_OVERFLOW, not demodulated -- then a normal burst that
    decodes."""
    torch = torch_cuda
    C = 1 << 24
    rx = LiveReceiver(2, 40, max_burst_len=65536, max_chunk_len=C, device=DEV)
    out = rx.alloc_result()
    loud = torch.zeros((2, C), dtype=torch.int16, device=DEV)
    loud[1] = 20000
    tr = afskmodem.Transmitter(1200, 0.1)
    closed = torch.zeros((), dtype=torch.int64, device=DEV)
    got = [[], []]
    state = {"pos": 0}

    def quiet_to(target, src):
        while state["pos"] < target:
            t = min(C, target - state["pos"])
            rx.push(src[:, :t], out=out)
            closed.add_(out.n_closed.sum())
            state["pos"] += t

    def push_capture(cap, sizes):
        d = torch.from_numpy(cap).to(DEV)
        p = 0
        for t in sizes:
            collect(rx.push(d[:, p: p + t]), got)
            p += t
        assert p == cap.shape[1]
        state["pos"] += p

    quiet_to(C, torch.zeros_like(loud))                     # the first chunk quiet on both channels
    quiet_to((1 << 31) - 3 * BLOCK - 1, loud)               # channel 1 loud from sample C on
    assert closed.item() == 0
    # capture A from the odd position P0: channel 0 bursts at 2^31 - 4096 (straddling 2^31) and 2^31 + 24576
    P0 = state["pos"]
    wa, wb = tr.wav_samples(b"straddles 2^31"), tr.wav_samples(b"after 2^31")
    sa, sb = (1 << 31) - 2 * BLOCK, (1 << 31) + 12 * BLOCK
    assert sa < 1 << 31 < sa + len(wa) - 4800 and sa + len(wa) + 2 * BLOCK <= sb
    la = sb + len(wb) + 3 * BLOCK - P0
    cap = np.zeros((2, la), np.int16)
    cap[0, sa - P0: sa - P0 + len(wa)] = wa
    cap[0, sb - P0: sb - P0 + len(wb)] = wb
    cap[1] = 20000
    push_capture(cap, [1, 2047, 2049, 8191] + [4097] * ((la - 12288) // 4097) + [(la - 12288) % 4097])
    win_a = (P0 - P0 % BLOCK, np.concatenate([np.zeros(P0 % BLOCK, np.int16), cap[0]]))
    # channel 1 stays loud until E, past 2^31 samples of loud; capture B from the odd position P1: channel 0 a burst
    # straddling 2^32, channel 1 quiet from E on and a normal burst at S4
    quiet_to((1 << 32) - 3 * BLOCK - 1, loud)
    assert closed.item() == 0
    P1 = state["pos"]
    wc, wd = tr.wav_samples(b"straddles 2^32"), tr.wav_samples(b"decodes after the overflow")
    sc, E = (1 << 32) - 2 * BLOCK, (1 << 32) - BLOCK
    S4 = E + 6 * BLOCK
    assert sc < 1 << 32 < sc + len(wc) - 4800 and E - C > 1 << 31
    lb = max(sc + len(wc), S4 + len(wd)) + 3 * BLOCK - P1
    cap = np.zeros((2, lb), np.int16)
    cap[0, sc - P1: sc - P1 + len(wc)] = wc
    cap[1, : E - P1] = 20000
    cap[1, S4 - P1: S4 - P1 + len(wd)] = wd
    push_capture(cap, [2049, 1, 2047] + [8192] * ((lb - 4097) // 8192) + [(lb - 4097) % 8192])
    win_b = (P1 - P1 % BLOCK, np.concatenate([np.zeros(P1 % BLOCK, np.int16), cap[0]]))
    win_c = (E + BLOCK, cap[1, E + BLOCK - P1:])            # after the closing block and the discarded one
    res = rx.flush()
    collect(res, got)
    torch.cuda.synchronize()
    # channel 0 against the oracle on block-aligned windows of the stream
    want0 = []
    for base, w in (win_a, win_b):
        for s, ln, f in oracle_bursts(w, 18000, 14000):
            d = O.demod_batch(w, np.array([s], np.int64), np.array([ln], np.int32), np.array([40], np.int32), 14000,
                              out_stride=rx.out_stride)
            want0.append(dict(channel=0, start=base + s, len=ln, flags=f,
                              bytes=d["bytes"][0, : int(d["nbytes"][0])].tobytes(),
                              **{k: int(d[k][0]) for k in FIELDS}))
    assert got[0] == want0
    assert [g["start"] for g in got[0]] == [sa, sb, sc]
    assert [g["bytes"] for g in got[0]] == [b"straddles 2^31", b"after 2^31", b"straddles 2^32"]
    # channel 1: the loud burst, clamped and flagged, not demodulated; then the normal burst
    big = got[1][0]
    assert (big["start"], big["len"], big["flags"]) == (C, (1 << 31) - BLOCK, _native.LIVE_OVERFLOW)
    assert big["status"] == _native.ST_TOO_SHORT and big["bytes"] == b"" and big["nbytes"] == 0
    base, w = win_c
    want1 = [(base + s, ln, f) for s, ln, f in oracle_bursts(w, 18000, 14000)]
    assert [(g["start"], g["len"], g["flags"]) for g in got[1][1:]] == want1 and want1[0][0] == S4
    assert [g["bytes"] for g in got[1][1:]] == [b"decodes after the overflow"]
    rx.close()
