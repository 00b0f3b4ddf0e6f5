"""GPU parity (-m gpu) of the streaming receiver's payload tap (LiveReceiver(max_burst_len=None, progressive=True),
afsk_live_push_tap).  Expected values never come from a live object alone: the CPU oracle's gate (gate_stream) and
demod (demod_batch, with a stride that holds the whole payload) over the concatenated capture, the tap model
(tests/live_tap_model.py) block by block for what must have arrived after every push, and the payloads a
LiveTransmitter sent.  Every push also goes through an untapped streaming receiver: every other output is equal."""
import functools

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from oracle import afsk_oracle as O
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import BLOCK, capture_of, noisy, push_sizes
from tests.live_tap_model import TapChannelModel, tap_cap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = [1, 7, 2047, 2048, 2049, 5000, 8192]                # what a "random" chunking draws its push sizes from
GUARD = 0xA5


def stack(caps):
    host = np.zeros((len(caps), max(c.size for c in caps)), np.int16)
    for i, c in enumerate(caps):
        host[i, : c.size] = c
    return host


def expected(cap, bf, a_start=18000, a_end=14000):
    """The oracle's gate + demod of one channel's whole capture: (start, length, flags, every payload byte)."""
    want, oe = O.gate_stream(cap, a_start, a_end, 4096)
    out = []
    for j, (s, n) in enumerate(want):
        stride = n // (14 * bf) + 2
        r = O.demod_batch(cap[s: s + n], [0], [n], [bf], a_end, out_stride=stride)
        nb = int(r["nbytes"][0])
        assert nb <= stride
        out.append((s, n, _native.LIVE_OPEN_END if (oe and j == len(want) - 1) else 0, r["bytes"][0, :nb].tobytes()))
    return out


def timeline(cap, bf, a_start=18000, a_end=14000):
    """The tap model's (open_start, open_nbytes) after every whole block of the capture: [blocks + 1] arrays."""
    ch = TapChannelModel(bf, a_start, a_end, 0)
    nb = cap.size // BLOCK
    os_, on = np.full(nb + 1, -1, np.int64), np.zeros(nb + 1, np.int64)
    for b in range(nb):
        r = ch.push(cap[b * BLOCK:(b + 1) * BLOCK])
        os_[b + 1], on[b + 1] = r["open_start"], r["open_nbytes"]
    return os_, on


EXISTING = ("n_closed", "burst_start", "burst_len", "flags")
DEMOD = ("bytes", "nbytes", "nbits", "clock_idx", "term_frame", "status", "corrected")


def run(torch, host, bfs, sizes, maxp, a=(18000, 14000), lines=None, flush=True, every_push=True, reset_at=None):
    """Push `host` in chunks of `sizes` (then flush) through a tapped receiver and an untapped one.  Returns
    (events per push, assembled bursts, max tap_n per channel); asserts on the way that every existing output of the
    two is equal, tap_n <= tap_cap, nothing is written behind tap_n, and -- with `lines`, the model's timelines per
    channel -- that open_start / open_nbytes after every push are the model's for the blocks pushed so far.
    reset_at: (push index, mask) -- both receivers reset(mask) before that push."""
    n, total = host.shape
    d = torch.from_numpy(host).to(DEV)
    kw = dict(max_burst_len=None, max_payload_len=maxp, max_chunk_len=max(max(sizes), 1), device=DEV)
    tapped = LiveReceiver(n, bfs, a[0], a[1], progressive=True, **kw)
    plain = LiveReceiver(n, bfs, a[0], a[1], **kw)
    assert tapped.tap_cap == tap_cap(kw["max_chunk_len"], int(np.min(bfs)))
    assert tapped.state_bytes == plain.state_bytes and tapped.slots == plain.slots
    out_t, out_u = tapped.alloc_result(diagnostics=True), plain.alloc_result(diagnostics=True)
    assert out_u.tap is None
    out_t.tap.bytes.fill_(GUARD)
    bad = torch.zeros((), dtype=torch.bool, device=DEV)
    asm = tapped.assembler()
    events, done = [], []
    maxn = np.zeros(n, np.int64)
    p = 0
    steps = [(t, False) for t in sizes] + ([(0, True)] if flush else [])
    for i, (t, fl) in enumerate(steps):
        if reset_at is not None and reset_at[0] == i:
            tapped.reset(reset_at[1])
            plain.reset(reset_at[1])
            asm.drop(reset_at[1])
        tapped.push(d[:, p: p + t], out=out_t, flush=fl)
        plain.push(d[:, p: p + t], out=out_u, flush=fl)
        p += t
        tp = out_t.tap
        small = torch.stack([tp.n.long(), out_t.n_closed.long(), out_u.n_closed.long(), tp.open_start,
                             tp.open_nbytes.long()]).cpu().numpy()
        assert (small[0] <= tapped.tap_cap).all() and (small[0] >= 0).all()
        maxn = np.maximum(maxn, small[0])
        busy = bool(small[:3].any())
        if every_push or busy or i % 997 == 0:
            for f in EXISTING:
                bad |= (getattr(out_t, f) != getattr(out_u, f)).any()
            for f in DEMOD:
                bad |= (getattr(out_t.demod, f) != getattr(out_u.demod, f)).any()
        if fl:
            assert (small[3] == -1).all() and (small[4] == 0).all()          # a flush leaves nothing open
        elif lines is not None:
            b = p // BLOCK
            for c, (os_, on) in enumerate(lines):
                assert (small[3][c], small[4][c]) == (os_[b], on[b]), (c, i, p)
        if busy:
            ev = out_t.partials()
            events.append(ev)
            done += asm.feed(out_t)
            # the row layout: the slots' shares, then the open burst's
            tl = tp.len.cpu().numpy()
            for c in range(n):
                k = int(small[1][c])
                assert (tl[c, k:] == 0).all() and tl[c, :k].sum() <= small[0][c]
                if small[3][c] < 0:
                    assert tl[c, :k].sum() == small[0][c]
        else:
            events.append([])
    assert p == total
    assert not bool(bad), "an existing output differs from the untapped receiver's"
    rows = out_t.tap.bytes.cpu().numpy()
    for c in range(n):
        assert (rows[c, int(maxn[c]):] == GUARD).all(), c
    assert asm.pending() == {} or not flush
    tapped.close()
    plain.close()
    return events, done, maxn


def check_events(events, done, want_by_channel):
    """Every burst's segments: offsets contiguous from 0, one final segment (the last), the bytes the oracle's; the
    assembler's bursts are the oracle's with their whole payloads."""
    seg = {}
    order = {}
    for ev in events:
        for c, start, offset, data, final in ev:
            s = seg.setdefault((c, start), dict(data=bytearray(), finals=0))
            assert s["finals"] == 0, (c, start, "a segment after the final one")
            assert offset == len(s["data"]), (c, start, offset, len(s["data"]))
            s["data"] += data
            s["finals"] += int(final)
            if final:
                order.setdefault(c, []).append(start)
    by = want_by_channel if isinstance(want_by_channel, dict) else dict(enumerate(want_by_channel))
    for c, want in by.items():
        assert order.get(c, []) == [w[0] for w in want], c
        for start, length, flags, payload in want:
            s = seg.pop((c, start))
            assert s["finals"] == 1 and bytes(s["data"]) == payload, (c, start, len(s["data"]), len(payload))
        assert [b for b in done if b[0] == c] == [(c, w[0], w[1], w[3]) for w in want], c
    assert not seg, list(seg)


CASES = {"1200_256": (40, 256), "1200_2000": (40, 2000), "300_64": (160, 64), "24_8": (2000, 8),
         "6000_long": (8, 66000)}


@functools.lru_cache(maxsize=None)
def case(name):
    """Two channels: the case's long payload followed by a short message, and three medium messages."""
    bf, plen = CASES[name]
    rng = np.random.default_rng(plen + bf)
    pay = bytes(rng.integers(0, 256, plen, dtype=np.uint8))
    training = 0.1 if name != "24_8" else 0.5
    caps = [capture_of(rng, bf, [pay, b"short"], training=training),
            capture_of(rng, bf, [bytes(rng.integers(0, 256, max(1, min(plen, 600) // 3), dtype=np.uint8))
                                 for _ in range(3)], training=training)]
    host = stack(caps)
    want = [expected(host[c], bf) for c in range(2)]
    assert want[0][0][3] == pay and len(want[0]) == 2 and len(want[1]) == 3, name
    return bf, host, want, [timeline(host[c], bf) for c in range(2)]


@pytest.mark.parametrize("maxp", [0, 16])
@pytest.mark.parametrize("T", [1, 7, 2047, 2048, 2049, 8192, 48000, "random"])
def test_reassembly_and_timeliness(torch_cuda, T, maxp):
    """256 B and 2000 B at 1200 baud, 64 B at 300 baud, 8 B at 24 baud and 66000 B (more than afsk_live_stream_layout's
    max_payload_len cap) at 6000 baud, with payload rows of 0 and 16 bytes: the segments of every burst put together
    are the oracle's bytes, and after every push the open burst's start and byte count are the model's.  (One push
    per sample or seven: the 256-byte 1200-baud case only, as in tests/test_gpu_live_stream.py.)"""
    names = ("1200_256",) if T in (1, 7) else tuple(CASES)
    for name in names:
        bf, host, want, lines = case(name)
        rng = np.random.default_rng(11)
        sizes = push_sizes(T, host.shape[1], rng, STEPS)
        events, done, maxn = run(torch_cuda, host, bf, sizes, maxp, lines=lines, every_push=T not in (1, 7))
        check_events(events, done, want)
        if name == "6000_long":
            assert len(want[0][0][3]) > 65536
        # the payload arrived while the burst was recording: over many pushes, not in the last one
        if T != 48000 or name in ("1200_2000", "6000_long", "24_8"):
            n_seg = sum(1 for ev in events for e in ev if e[0] == 0 and e[1] == want[0][0][0] and e[3])
            assert n_seg >= 3, (name, n_seg)


def test_several_bursts_of_one_channel_in_one_push(torch_cuda):
    """T = 48000, short messages at 2400 baud: several slots of one push carry bytes, tap_len per slot is the burst's
    own count, and the open burst's remainder follows them."""
    rng = np.random.default_rng(21)
    pays = [[bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)) for _ in range(14)] for _ in range(3)]
    host = stack([capture_of(rng, 20, p, gap=2 * BLOCK, training=0.1) for p in pays])
    want = [expected(host[c], 20) for c in range(3)]
    events, done, _ = run(torch_cuda, host, 20, push_sizes(48000, host.shape[1], rng, STEPS), 0,
                          lines=[timeline(host[c], 20) for c in range(3)])
    check_events(events, done, want)
    for c in range(3):
        assert [w[3] for w in want[c]] == pays[c], c
    per_push = [sum(1 for e in ev if e[0] == 0 and e[4] and e[3]) for ev in events]
    assert max(per_push) >= 2
    assert any(any(e[4] for e in ev) and any(not e[4] for e in ev) for ev in events)      # slots and an open remainder


def test_bursts_that_decode_nothing(torch_cuda):
    """Too short, no terminator, squelched at once: no tap byte, one final segment with b"" per reported burst."""
    rng = np.random.default_rng(22)
    total = 60 * BLOCK
    host = np.zeros((4, total), np.int16)
    for b in range(2, 56, 3):
        host[0, b * BLOCK:(b + 1) * BLOCK] = 30000                              # one-block bursts: TOO_SHORT
    tr = np.tile(O.training_cycle(1200).astype(np.int16), 40 * BLOCK // 80)
    host[1, 3 * BLOCK: 3 * BLOCK + tr.size] = tr                                # training only: no terminator
    w = afskmodem.Transmitter(1200, 0.2).wav_samples(b"never decoded")
    cut = int(0.2 * 48000) + 4 * 40 + 3
    host[2, 2 * BLOCK: 2 * BLOCK + cut] = w[:cut]                               # silence right behind the terminator
    host[2, 2 * BLOCK + cut: 8 * BLOCK] = 0
    host[3] = noisy(rng, np.zeros(total), 12000.0)
    want = [expected(host[c], 40) for c in range(4)]
    assert len(want[0]) >= 15 and all(w[3] == b"" for c in (0, 1, 2) for w in want[c]) and want[1] and want[2]
    for T in (8192, 2049):
        events, done, maxn = run(torch_cuda, host, 40, push_sizes(T, total, rng, STEPS), 0,
                                 lines=[timeline(host[c], 40) for c in range(4)])
        check_events(events, done, want)
        assert (maxn[:3] == 0).all()
        assert all(e[3] == b"" and e[4] for ev in events for e in ev if e[0] < 3)


def test_mixed_rates_and_a_threshold_pair_per_channel(torch_cuda):
    """The tapped thr kernel: every channel equals the oracle at its rate and pair, and a one-rate, one-pair tapped
    receiver's segments."""
    rng = np.random.default_rng(23)
    bfs = [40, 8, 160, 20, 40, 2000, 80, 12]
    starts = [18000, 12000, 20000, 18000, 9000, 18000, 15000, 18000]
    ends = [14000, 8000, 14000, 6000, 5000, 14000, 11000, 14000]
    pays = [[bytes(rng.integers(0, 256, int(rng.integers(2, 20 if bf < 1000 else 4)), dtype=np.uint8))
             for _ in range(2)] for bf in bfs]
    caps = [capture_of(rng, bf, p, sigma=1500.0, training=max(0.05, 3.0 * bf / 48000)) for bf, p in zip(bfs, pays)]
    host = stack(caps)
    sizes = push_sizes(8192, host.shape[1], rng, STEPS)
    want = [expected(host[c], bfs[c], starts[c], ends[c]) for c in range(len(bfs))]
    lines = [timeline(host[c], bfs[c], starts[c], ends[c]) for c in range(len(bfs))]
    events, done, _ = run(torch_cuda, host, bfs, sizes, 4, a=(starts, ends), lines=lines)
    check_events(events, done, want)
    assert sum(len(w[3]) > 0 for ws in want for w in ws) >= len(bfs)
    for c in (1, 4, 5):
        ev1, done1, _ = run(torch_cuda, host[c:c + 1], bfs[c], sizes, 4, a=(starts[c], ends[c]))
        mine = [[(0,) + e[1:] for e in ev if e[0] == c] for ev in events]
        assert mine == ev1, c


def test_reset_with_a_mask_in_mid_burst(torch_cuda):
    rng = np.random.default_rng(24)
    n = 6
    pay = bytes(rng.integers(0, 256, 120, dtype=np.uint8))
    w = afskmodem.Transmitter(1200, 0.1).wav_samples(pay)
    host = np.zeros((n, 4 * BLOCK + w.size + 4 * BLOCK), np.int16)
    host[:, 4 * BLOCK: 4 * BLOCK + w.size] = w
    T = 4096
    sizes = push_sizes(T, host.shape[1], rng, STEPS)
    at = (4 * BLOCK + w.size // 2) // T                         # a push in mid-payload
    mask = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    events, done, _ = run(torch_cuda, host, 40, sizes, 0, reset_at=(at, mask))
    before = [e for ev in events[:at] for e in ev]
    assert {e[0] for e in before} == set(range(n)) and all(not e[4] for e in before)
    # a dropped channel starts a new stream at the reset: what the oracle gates in the rest of the capture, and
    # nothing more of the burst that was open
    for c in range(n):
        after = [e for ev in events[at:] for e in ev if e[0] == c]
        if mask[c]:
            want = expected(host[c, at * T:], 40)
            assert all(e[1] != 4 * BLOCK for e in after), c
            segs = {}
            for e in after:
                segs.setdefault(e[1], bytearray()).extend(e[3])
            assert [(e[1], bytes(segs[e[1]])) for e in after if e[4]] == [(x[0], x[3]) for x in want], c
            assert [b[1:] for b in done if b[0] == c] == [(x[0], x[1], x[3]) for x in want], c
        else:
            assert [b[1:] for b in done if b[0] == c] == [(4 * BLOCK, b[2], pay) for b in done if b[0] == c], c
            assert len([b for b in done if b[0] == c]) == 1
    # open_start right after the reset push: -1 for the dropped channels (their rest of the message does not start a
    # burst within one push: the discard block, then the start block), the burst's start for the others
    rx = LiveReceiver(n, 40, max_burst_len=None, max_payload_len=0, max_chunk_len=T, device=DEV, progressive=True)
    d = torch_cuda.from_numpy(host).to(DEV)
    out = rx.alloc_result()
    for i in range(at):
        rx.push(d[:, i * T:(i + 1) * T], out=out)
    assert (out.tap.open_start.cpu().numpy() == 4 * BLOCK).all() and (out.tap.open_nbytes.cpu().numpy() > 0).all()
    rx.reset(mask)
    rx.push(d[:, at * T: at * T + BLOCK], out=out)
    assert out.tap.open_start.cpu().numpy().tolist() == [-1 if m else 4 * BLOCK for m in mask]
    assert (out.tap.n.cpu().numpy()[mask == 1] == 0).all() and (out.tap.open_nbytes.cpu().numpy()[mask == 1] == 0).all()
    rx.close()


def test_graph_captured_tapped_push_matches_eager(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(25)
    n, T = 32, 4096
    bfs = [(8, 20, 40, 80, 160, 400)[i % 6] for i in range(n)]
    caps = [capture_of(rng, bf, [bytes(rng.integers(0, 256, 30 if bf <= 80 else 3, dtype=np.uint8))],
                       training=max(0.02, 3.0 * bf / 48000)) for bf in bfs]
    host = stack(caps)
    total = -(-host.shape[1] // T) * T
    host = np.concatenate([host, np.zeros((n, total - host.shape[1]), np.int16)], axis=1)
    d = torch.from_numpy(host).to(DEV)
    kw = dict(max_burst_len=None, max_payload_len=0, max_chunk_len=T, device=DEV, progressive=True)
    eager, graphed = LiveReceiver(n, bfs, **kw), LiveReceiver(n, bfs, **kw)
    src = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    out_g, out_e = graphed.alloc_result(), eager.alloc_result()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graphed.push(src, out=out_g, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    graphed.reset()
    ev_e, ev_g = [], []
    asm = graphed.assembler()
    done = []
    for p in range(0, total, T):
        src.copy_(d[:, p: p + T])
        g.replay()
        ev_g.append(out_g.partials())
        done += asm.feed(out_g)
        ev_e.append(eager.push(d[:, p: p + T], out=out_e).partials())
        for a, b in zip((out_g.tap.n, out_g.tap.len, out_g.tap.open_start, out_g.tap.open_nbytes),
                        (out_e.tap.n, out_e.tap.len, out_e.tap.open_start, out_e.tap.open_nbytes)):
            assert torch.equal(a, b)
    assert ev_e == ev_g
    want = [expected(host[c], bfs[c]) for c in range(n)]
    for c in range(n):
        assert [b[1:] for b in done if b[0] == c] == [(w[0], w[1], w[3]) for w in want[c]], c
    assert sum(len(b[3]) > 0 for b in done) >= n // 2
    eager.close()
    graphed.close()


def test_loopback_16384_channels_256_byte_messages(torch_cuda):
    """LiveTransmitter.pull into push: with payload rows of 0 bytes the assembler returns every 256-byte payload."""
    torch = torch_cuda
    rng = np.random.default_rng(26)
    n, T = 16384, 8192
    tx = LiveTransmitter(n, 1200, 0.1, max_payload_len=256, device=DEV)
    rx = LiveReceiver(n, 40, max_burst_len=None, max_payload_len=0, max_chunk_len=T, device=DEV, progressive=True)
    pays = [bytes(rng.integers(0, 256, 256, dtype=np.uint8)) for _ in range(n)]
    tx.submit(np.arange(n), pays)
    longest = int(np.max(tx.message_len(256))) + 4 * T
    buf = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    out = rx.alloc_result()
    asm = rx.assembler()
    done = asm.feed(rx.push(torch.zeros((n, T), dtype=torch.int16, device=DEV), out=out))      # (the discard block)
    early = 0
    for _ in range(0, longest, T):
        tx.pull(T, out=buf)
        done += asm.feed(rx.push(buf, out=out))
        early = max(early, len(asm.pending()))
        assert int(out.tap.n.max()) <= rx.tap_cap
    done += asm.feed(rx.flush(out=out))
    assert early == n                                           # every channel had bytes before its burst closed
    assert sorted((b[0], b[3]) for b in done) == [(c, pays[c]) for c in range(n)]
    tx.close()
    rx.close()


def test_full_size_65536_channels_8192(torch_cuda):
    """65536 channels x 4 pushes of 8192: tap_n <= tap_cap everywhere, nothing behind tap_n is written (the rows start
    as a guard pattern, so a store past a row's end would show in its neighbour), a seeded sample against the oracle."""
    torch = torch_cuda
    rng = np.random.default_rng(27)
    n, T = 65536, 8192
    pay = bytes(rng.integers(0, 256, 24, dtype=np.uint8))
    w = afskmodem.Transmitter(1200, 0.05).wav_samples(pay)
    total = 4 * T
    row = np.zeros(total, np.int16)
    row[T // 2: T // 2 + w.size] = w
    shifts = rng.integers(0, 2 * BLOCK, n)
    d = torch.from_numpy(row).to(DEV).repeat(n, 1)
    idx = (torch.arange(total, device=DEV)[None, :] - torch.from_numpy(shifts).to(DEV)[:, None]) % total
    d = torch.gather(d, 1, idx)
    rx = LiveReceiver(n, 40, max_burst_len=None, max_payload_len=0, max_chunk_len=T, device=DEV, progressive=True)
    assert rx.tap_cap == 19
    out = rx.alloc_result()
    asm = rx.assembler()
    done = []
    col = torch.arange(rx.tap_cap, device=DEV)[None, :]
    sample = sorted(rng.choice(n, 64, replace=False).tolist())
    events = {c: [] for c in sample}
    for i, p in enumerate(list(range(0, total, T)) + [None]):
        out.tap.bytes.fill_(GUARD)
        if p is None:
            rx.flush(out=out)
        else:
            rx.push(d[:, p: p + T], out=out)
        tn = out.tap.n
        assert int(tn.max()) <= rx.tap_cap and int(tn.min()) >= 0
        assert not bool(((out.tap.bytes != GUARD) & (col >= tn[:, None])).any())
        assert int(out.tap.len.sum(dim=1).sub(tn).max()) <= 0
        for e in out.partials():
            if e[0] in events:
                events[e[0]].append(e)
        done += asm.feed(out)
    host = d[torch.as_tensor(sample, device=DEV)].cpu().numpy()
    by_channel = {}
    for b in done:
        by_channel.setdefault(b[0], []).append(b)
    for j, c in enumerate(sample):
        want = expected(host[j], 40)
        check_events([events[c]], by_channel.get(c, []), {c: want})
    assert all(any(b[3] == pay for b in by_channel.get(c, [])) for c in range(n))
    rx.close()
