"""GPU parity (-m gpu) of the live transmitter (afsk_live_tx_*, ``LiveTransmitter``): pulled chunk by chunk, every
channel must carry exactly the samples ``Transmitter.wav_samples`` makes of its queued messages, where the queue
model (tests/live_tx_model.py) puts them -- the reference's own frame digests, seeded queueing against the model,
column windows, reset, graph replay, and a loopback through ``LiveReceiver``.  Expected values never come from the
live path itself."""
import ctypes as C

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, synth
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests.golden_inputs import sha_i16
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import random_payload
from tests.live_tx_model import LiveTxModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def sizes_for(kind, total, rng):
    """Pull sizes summing to total."""
    if kind == "whole":
        return [total]
    if kind == "ragged":
        out, left = [], total
        while left > 0:
            t = min(int(rng.choice([0, 1, 3, 7, 4095, 4096, 4097, 4801, 9000, 20000])), left)
            out.append(t)
            left -= t
        return out
    if kind == "1":
        # one sample at a time over the first 6000 samples (the start, odd phases, the first tone boundaries), then
        # the rest in odd-sized chunks
        head = min(6000, total)
        return [1] * head + [min(4801, total - p) for p in range(head, total, 4801)]
    step = int(kind)
    return [min(step, total - p) for p in range(0, total, step)]


def pull_into(tx, buf, sizes, first=0):
    pos = first
    for t in sizes:
        tx.pull(t, out=buf[:, pos: pos + t] if t else buf[:, pos: pos + 1])
        pos += t
    return pos


def wav_cache(baud, training_time):
    tr = afskmodem.Transmitter(baud, training_time)
    cache = {}

    def wav(p):
        if p not in cache:
            cache[p] = tr.wav_samples(p)
        return cache[p]
    return wav


def digest_groups(golden):
    groups = {}
    for c in golden["frames"]:
        groups.setdefault((c["baud"], c["training_time"]), []).append(
            (bytes.fromhex(c["payload_hex"]), c["n_wav"], c["wav_sha256"]))
    for c in golden["degenerate_api"]["training_time"]:
        groups.setdefault((c["baud"], c["training_time"]), []).append((b"Hi!", c["n_wav"], c["wav_sha256"]))
    return groups


@pytest.mark.parametrize("kind", ["whole", "1", "7", "2048", "4801", "48000", "ragged"])
def test_reference_digests_in_every_chunking(golden, torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(23)
    groups = digest_groups(golden)
    assert sum(len(v) for v in groups.values()) == 72 + len(golden["degenerate_api"]["training_time"])
    for (baud, tt), cases in groups.items():
        n = len(cases)
        tx = LiveTransmitter(n, baud, tt, queue_depth=2, max_payload_len=max(len(p) for p, _, _ in cases),
                             device=DEV)
        # a lead of 3 samples (whole: none) puts every message at an odd stream index
        lead = 0 if kind == "whole" else 3
        total = lead + max(w for _, w, _ in cases) + 4096
        buf = torch.full((n, total), 12345, dtype=torch.int16, device=DEV)
        pos = pull_into(tx, buf, [lead] if lead else [])
        res = tx.submit(list(range(n)), [p for p, _, _ in cases])
        status, start, ns = res.cpu()
        assert (status == _native.LIVE_TX_QUEUED).all() and (start == lead).all()
        assert ns.tolist() == [w for _, w, _ in cases]
        pull_into(tx, buf, sizes_for(kind, total - pos, rng), pos)
        assert tx.pending.cpu().numpy().tolist() == [0] * n
        host = buf.cpu().numpy()
        for c, (p, n_wav, sha) in enumerate(cases):
            assert sha_i16(host[c, lead: lead + n_wav]) == sha, (baud, tt, p, kind)
            assert not host[c, :lead].any() and not host[c, lead + n_wav:].any(), (baud, tt, p, kind)
        torch.cuda.synchronize()
        tx.close()


def test_seeded_queueing_against_the_model(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n, depth, mp = 4096, 3, 24
    tx = LiveTransmitter(n, 1200, 0.1, queue_depth=depth, max_payload_len=mp, device=DEV)
    model = LiveTxModel(n, tx.bit_frames, tx.ts_cycles, depth, mp, wav=wav_cache(1200, 0.1))
    for rnd in range(14):
        k = int(rng.integers(0, 3 * n))
        chans = rng.integers(0, n, k)
        bad = rng.random(k) < 0.02
        chans[bad] = rng.choice([-1, n, n + 5, -7], int(bad.sum()))
        pays = [random_payload(rng, 0, mp + 4) if rng.random() < 0.05 else random_payload(rng, 0, mp)
                for _ in range(k)]
        if rng.random() < 0.2:                              # idle rounds: nothing queued
            chans, pays = chans[:0], []
        res = tx.submit(chans, pays)
        want = model.submit(chans, pays)
        for g, w, name in zip(res.cpu(), want, ("status", "start", "n_samples")):
            assert (g == w).all(), (rnd, name, np.nonzero(g != w)[0][:5])
        for _ in range(int(rng.integers(1, 4))):
            T = int(rng.choice([0, 1, 7, 4095, 4096, 4097, 5000, 8192, 12345, 30000]))
            out = tx.pull(T)
            exp = model.expected(T)
            pend = model.pull(T)
            got = out.cpu().numpy()
            bad = np.nonzero((got != exp).any(axis=1))[0]
            assert bad.size == 0, (rnd, T, bad[:5])
            assert (tx.pending.cpu().numpy() == pend).all(), rnd
    torch.cuda.synchronize()
    tx.close()


def test_statuses_are_all_reached(torch_cuda):
    torch = torch_cuda
    tx = LiveTransmitter(4, 2400, 0.0, queue_depth=2, max_payload_len=3, device=DEV)
    res = tx.submit([3, 0, 9, 0, 0, 3], [b"a", b"", b"", b"abcd", b"xyz", b"q"])
    st, s, ns = res.cpu()
    assert st.tolist() == [_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUED, _native.LIVE_TX_BAD_CHANNEL,
                           _native.LIVE_TX_TOO_LONG, _native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUED]
    m = LiveTxModel(4, 20, 0, 2, 3)
    assert s.tolist() == m.submit([3, 0, 9, 0, 0, 3], [b"a", b"", b"", b"abcd", b"xyz", b"q"])[1].tolist()
    st, _, _ = tx.submit([0], [b""]).cpu()
    assert st.tolist() == [_native.LIVE_TX_QUEUE_FULL]
    torch.cuda.synchronize()
    tx.close()


def test_pull_writes_exactly_its_column_window(torch_cuda):
    torch = torch_cuda
    n, T, S = 37, 5001, -31111
    tx = LiveTransmitter(n, 1200, 0.0, device=DEV)
    model = LiveTxModel(n, 40, 0, 4, 256, wav=wav_cache(1200, 0.0))
    rng = np.random.default_rng(3)
    pays = [random_payload(rng, 0, 40) for _ in range(n)]
    tx.submit(range(n), pays)
    model.submit(range(n), pays)
    buf = torch.full((n, 3 * T + 5), S, dtype=torch.int16, device=DEV)
    for a in (1, T + 2, 2 * T + 3):                          # odd column offsets: 2-byte aligned rows
        before = buf.cpu().numpy()
        tx.pull(T, out=buf[:, a: a + T])
        exp = model.expected(T)
        model.pull(T)
        after = buf.cpu().numpy()
        assert (after[:, a: a + T] == exp).all()
        outside = np.ones(after.shape[1], bool)
        outside[a: a + T] = False
        assert (after[:, outside] == before[:, outside]).all()
    assert (buf.cpu().numpy()[:, 0] == S).all() and (buf.cpu().numpy()[:, -2:] == S).all()
    torch.cuda.synchronize()
    tx.close()


def test_reset_mid_message(torch_cuda):
    torch = torch_cuda
    n = 64
    tx = LiveTransmitter(n, 1200, 0.5, device=DEV)
    model = LiveTxModel(n, 40, tx.ts_cycles, 4, 256, wav=wav_cache(1200, 0.5))
    rng = np.random.default_rng(9)
    pays = [random_payload(rng, 1, 30) for _ in range(2 * n)]
    chans = np.repeat(np.arange(n), 2)
    tx.submit(chans, pays)
    model.submit(chans, pays)
    for T in (10001, 9000):
        assert (tx.pull(T).cpu().numpy() == model.expected(T)).all()
        model.pull(T)
    mask = np.arange(n) % 3 == 0
    tx.reset(torch.from_numpy(mask).to(DEV))
    model.reset(mask)
    assert (tx.pending.cpu().numpy() == model.pending()).all()
    assert (tx.pending.cpu().numpy()[mask] == 0).all()
    got = tx.pull(20000).cpu().numpy()
    assert not got[mask].any()                               # silenced from the next sample
    assert (got == model.expected(20000)).all()               # the others go on unaffected
    model.pull(20000)
    # the reset channels restarted at 0: a message queued now starts at 20000 of the new stream
    st, s, _ = tx.submit([0, 1], [b"a", b"b"]).cpu()
    ws, wst, _ = model.submit([0, 1], [b"a", b"b"])
    assert (st == ws).all() and s.tolist() == wst.tolist() and s[0] == 20000
    assert (tx.pull(30000).cpu().numpy() == model.expected(30000)).all()
    torch.cuda.synchronize()
    tx.close()


def test_graph_replay_equals_eager_pulls(torch_cuda):
    torch = torch_cuda
    n, T, K = 256, 3001, 12
    rng = np.random.default_rng(17)
    chans = np.repeat(np.arange(n), 3)
    pays = [random_payload(rng, 0, 20) for _ in range(3 * n)]
    eager = LiveTransmitter(n, 1200, 0.1, device=DEV)
    graphed = LiveTransmitter(n, 1200, 0.1, device=DEV)
    eager.submit(chans, pays)
    graphed.submit(chans, pays)
    want = [eager.pull(T).clone() for _ in range(K)]
    buf = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.pull(T, out=buf)
    for k in range(K):
        g.replay()
        assert torch.equal(buf, want[k]), k
    assert torch.equal(graphed.pending, eager.pending)
    torch.cuda.synchronize()
    del g
    eager.close()
    graphed.close()


def loopback(torch, n, per_channel, plen_max, training_time, snr_db, seed, chunk=8192):
    """Queue per_channel messages on every channel, pull [n, chunk] windows of a [n, total] buffer, (noise), push the
    same windows to a LiveReceiver, flush.  Returns (buffer, payloads per channel, bursts per channel)."""
    rng = np.random.default_rng(seed)
    tx = LiveTransmitter(n, 1200, training_time, queue_depth=per_channel, max_payload_len=plen_max, device=DEV)
    pays = [[random_payload(rng, 0, plen_max) for _ in range(per_channel)] for _ in range(n)]
    res = tx.submit(np.repeat(np.arange(n), per_channel), [p for row in pays for p in row])
    last_end = int((res.start + res.n_samples.to(torch.int64)).max().item())
    assert (res.status == _native.LIVE_TX_QUEUED).all().item()
    total = -(-(last_end + 2 * 2048) // chunk) * chunk
    buf = torch.empty((n, total), dtype=torch.int16, device=DEV)
    rx = LiveReceiver(n, 40, device=DEV, max_chunk_len=chunk)
    got = [[] for _ in range(n)]
    row_off = torch.arange(n, dtype=torch.int64, device=DEV) * total
    lens = torch.full((n,), chunk, dtype=torch.int32, device=DEV)
    scale = np.full(n, synth.snr_to_scale_q24(snr_db), np.int32) if snr_db is not None else None
    for k, pos in enumerate(range(0, total, chunk)):
        win = buf[:, pos: pos + chunk]
        tx.pull(chunk, out=win)
        if scale is not None:
            batch.add_noise_batch(buf.view(-1), row_off + pos, lens, chunk, scale, seed=seed * 1000 + k)
        r = rx.push(win, flush=pos + chunk == total)
        for c, _, _, data in r.bursts():
            got[c].append(data)
    assert (tx.pending == 0).all().item()
    torch.cuda.synchronize()
    tx.close()
    rx.close()
    return buf, pays, got


@pytest.mark.parametrize("snr_db", [None, 20.0])
def test_loopback_through_the_live_receiver(torch_cuda, snr_db):
    torch = torch_cuda
    n = 4096
    buf, pays, got = loopback(torch, n, 3, 64, 0.5, snr_db, seed=41 if snr_db is None else 43)
    host = buf.cpu().numpy()
    del buf
    want = afskmodem.Receiver(1200).decode_captures(list(host), max_bursts=8)
    assert got == want
    if snr_db is None:
        assert got == pays                                   # every payload, in order


def test_loopback_at_65536_channels(torch_cuda):
    torch = torch_cuda
    n = 65536
    buf, pays, got = loopback(torch, n, 2, 16, 0.25, None, seed=59)
    rng = np.random.default_rng(61)
    sample = np.sort(rng.choice(n, 384, replace=False))
    host = buf[torch.from_numpy(sample).to(DEV)].cpu().numpy()
    del buf
    want = afskmodem.Receiver(1200).decode_captures(list(host), max_bursts=8)
    assert [got[c] for c in sample.tolist()] == want


def test_refused_arguments(torch_cuda):
    torch = torch_cuda
    for baud in (4800, 8000):
        with pytest.raises(ValueError):
            LiveTransmitter(4, baud, device=DEV)
        with pytest.raises(ValueError):
            afskmodem.Transmitter(baud).live(4)
    for n in (0, -3):
        with pytest.raises(ValueError):
            LiveTransmitter(n, 1200, device=DEV)
    h = C.c_void_p()
    assert _native.lib().afsk_live_tx_create(4, 42, 0, 4, 256, C.byref(h)) == _native.E_INVALID_BAUD and not h
    assert _native.lib().afsk_live_tx_create(0, 40, 0, 4, 256, C.byref(h)) == _native.E_INVALID_ARG and not h
    n, T = 8, 100
    tx = LiveTransmitter(n, 1200, device=DEV)
    with pytest.raises(TypeError):
        tx.pull(T, out=torch.zeros((n, T), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        tx.pull(T, out=torch.zeros((n, T), dtype=torch.int16))          # host memory
    with pytest.raises(ValueError):
        tx.pull(T, out=torch.zeros((n + 1, T), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError):
        tx.pull(T, out=torch.zeros((n, T - 1), dtype=torch.int16, device=DEV))
    flat = torch.zeros(n * T, dtype=torch.int16, device=DEV)
    with pytest.raises(ValueError):
        tx.pull(T, out=flat.as_strided((n, T), (T - 1, 1)))             # overlapping rows
    with pytest.raises(ValueError):
        tx.pull(T, out=torch.zeros((n, 2 * T), dtype=torch.int16, device=DEV)[:, ::2])   # non-contiguous rows
    with pytest.raises(ValueError):
        tx.pull(-1)
    assert _native.lib().afsk_live_tx_pull(tx.handle, None, 0, -1, tx.pending.data_ptr(), None) == \
        _native.E_INVALID_ARG
    assert _native.lib().afsk_live_tx_pull(tx.handle, flat.data_ptr(), T - 1, T, tx.pending.data_ptr(), None) == \
        _native.E_INVALID_ARG
    # the C entry: an unsorted channel array gets its status from the first message that breaks the order
    m = 4
    ch = torch.tensor([1, 0, 1, 2], dtype=torch.int32, device=DEV)
    off = torch.zeros(m, dtype=torch.int64, device=DEV)
    ln = torch.zeros(m, dtype=torch.int32, device=DEV)
    pay = torch.zeros(1, dtype=torch.uint8, device=DEV)
    st = torch.full((m,), -9, dtype=torch.int32, device=DEV)
    s = torch.full((m,), -9, dtype=torch.int64, device=DEV)
    ns = torch.full((m,), -9, dtype=torch.int32, device=DEV)
    _native.check(_native.lib().afsk_live_tx_submit(tx.handle, m, ch.data_ptr(), off.data_ptr(), ln.data_ptr(),
                                                    pay.data_ptr(), None, st.data_ptr(), s.data_ptr(), ns.data_ptr(),
                                                    None))
    torch.cuda.synchronize()
    U = _native.LIVE_TX_UNSORTED
    assert st.cpu().tolist() == [_native.LIVE_TX_QUEUED, U, U, U]
    assert s.cpu().tolist() == [0, -1, -1, -1] and ns.cpu().tolist()[1:] == [0, 0, 0]
    # T = 0 is a pull: it only writes pending
    tx.pull(0)
    torch.cuda.synchronize()
    assert tx.pending.cpu().tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    tx.close()
