"""GPU parity (-m gpu) of the auto-rate streaming live receiver (LiveReceiver(n, "auto"), afsk_live_create_stream_auto).
E1: with one candidate r it is, field for field, the fixed-rate streaming receiver at r.  E2: with any list, every burst
equals the fixed-rate answer at the rate the detector names for the burst's first 4096 samples -- expected values from
the oracle's gate over the whole capture, the detector's model and the oracle's demod (tests/live_auto_model.py), from
batch.detect_rates on the device, and from what was sent."""
import numpy as np
import pytest

from afskmodem_amd import _native, batch
from afskmodem_amd.live import LiveReceiver
from tests import live_auto_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import BLOCK, collect, drive, push_sizes, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = [1, 7, 2047, 2048, 2049, 5000, 8192]                # what a "random" chunking draws its push sizes from
TAP_FIELDS = ("bytes", "n", "len", "open_start", "open_nbytes")


def unused_slots_are_clear(res):
    nc = res.n_closed.cpu().numpy()
    bf, sc = res.bit_frames.cpu().numpy(), res.rate_score.cpu().numpy()
    for c in range(nc.size):
        assert not bf[c, nc[c]:].any() and (sc[c, nc[c]:] == -1).all(), c


def without_rates(rows):
    return [[{k: v for k, v in g.items() if k not in ("bit_frames", "rate_score")} for g in ch] for ch in rows]


@pytest.fixture(scope="module")
def rate_case():
    """Test 2's capture: three messages per channel at rotated rates, and what the model expects of every channel."""
    host, sent = M.rate_cases(M.SEED_RATES)
    return host, sent, [M.expected(cap) for cap in host]


# ------------------------------------------------------------------------------------------------------------- E1


@pytest.mark.parametrize("T", [2047, 2048, 2049, 8192, "random"])
@pytest.mark.parametrize("r", [8, 40, 160, 1000])
def test_one_candidate_equals_the_fixed_rate_streaming_receiver(torch_cuda, r, T):
    """The deciding block in the middle of a push (8192, random), at its very end (2048 and, while the carry is
    short, 2049), in a later push than block 0 (2047, 2048, random sizes 1 and 7)."""
    torch = torch_cuda
    rng = np.random.default_rng(1000 * r + (0 if T == "random" else T))
    n = 6
    pays = [[bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(2)] for _ in range(n)]
    host = M.stack([M.rated_capture(rng, [(r, p) for p in pays[c]] + [("block", 30000)]) for c in range(n)], BLOCK)
    host[:, -BLOCK:] = 30000                                   # one loud block before the flush: a TOO_SHORT burst
    d = torch.from_numpy(host).to(DEV)
    sizes = push_sizes(T, host.shape[1], rng, STEPS)
    fixed = LiveReceiver(n, r, max_burst_len=None, device=DEV)
    auto = LiveReceiver(n, "auto", candidates=[r], max_burst_len=None, device=DEV)
    assert auto.auto and auto.bit_frames is None and not auto.channel_bit_frames.any() and auto.candidates == (r,)
    assert auto.max_score is None and not fixed.auto and (auto.slots, auto.state_bytes) == (fixed.slots, fixed.state_bytes)
    want = drive(fixed, d, sizes, corrected=True)
    got = drive(auto, d, sizes, corrected=True, each=unused_slots_are_clear)
    fixed.close()
    auto.close()
    assert without_rates(got) == want
    for c in range(n):
        assert [g["bytes"] for g in got[c][:2]] == pays[c], c
        for g in got[c]:
            short = g["len"] < 4096
            assert g["bit_frames"] == (0 if short else r) and (g["rate_score"] == -1) == short, (c, g)
        assert got[c][-1]["status"] == _native.ST_TOO_SHORT and got[c][-1]["len"] == BLOCK


# ------------------------------------------------------------------------------------------------------------- E2


def check_rate_case(got, sent, want):
    for c in range(len(sent)):
        assert same(got[c], want[c]), c
        assert [(g["bit_frames"], g["bytes"]) for g in got[c]] == list(sent[c]), c
        assert all(g["status"] == _native.ST_OK and g["rate_score"] >= 0 for g in got[c]), c


@pytest.mark.parametrize("T", [8192, "random"])
def test_a_rate_per_burst_fast_slow_fast_on_one_channel(torch_cuda, rate_case, T):
    torch = torch_cuda
    host, sent, want = rate_case
    assert [bf for bf, _ in sent[0]] == [8, 1000, 20] and [bf for bf, _ in sent[1]] == [1000, 20, 160]
    rx = LiveReceiver(host.shape[0], "auto", max_burst_len=None, device=DEV)
    assert rx.candidates == batch.VALID_BIT_FRAMES
    got = drive(rx, torch.from_numpy(host).to(DEV), push_sizes(T, host.shape[1], np.random.default_rng(3), STEPS),
                each=unused_slots_are_clear)
    rx.close()
    check_rate_case(got, sent, want)


def test_the_reported_rate_score_and_clock_are_the_detectors(torch_cuda, rate_case):
    """The first 4096 samples of every reported burst, cut on the device, through batch.detect_rates."""
    torch = torch_cuda
    host, sent, _ = rate_case
    d = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(host.shape[0], "auto", max_burst_len=None, device=DEV)
    got = drive(rx, d, push_sizes(8192, host.shape[1]))
    rx.close()
    rows = [(c, g) for c in range(len(got)) for g in got[c]]
    assert len(rows) == 3 * host.shape[0]
    off = torch.tensor([c * host.shape[1] + g["start"] for c, g in rows], dtype=torch.int64, device=DEV)
    ln = torch.full((len(rows),), 4096, dtype=torch.int32, device=DEV)
    det = batch.detect_rates(d.reshape(-1), off, ln).cpu()
    for i, (c, g) in enumerate(rows):
        assert (g["bit_frames"], g["rate_score"], g["clock_idx"]) == \
            (int(det.bit_frames[i]), int(det.score[i]), int(det.clock_idx[i])), (c, g)


def test_more_than_one_blocks_worth_of_channels(torch_cuda):
    torch = torch_cuda
    host, sent = M.rate_cases(M.SEED_LARGE, M.LARGE_CHANNELS, 1)
    rx = LiveReceiver(M.LARGE_CHANNELS, "auto", max_burst_len=None, device=DEV)
    got = drive(rx, torch.from_numpy(host).to(DEV), push_sizes(8192, host.shape[1]))
    rx.close()
    check_rate_case(got, sent, [M.expected(cap) for cap in host])


# ------------------------------------------------------------------------------------- ties, max_score, short bursts


def test_the_earliest_candidate_wins_a_tie(torch_cuda):
    """A burst of constant +32767: every candidate scores 32767 at clock index 0."""
    torch = torch_cuda
    host = np.zeros((6, 16 * BLOCK), np.int16)
    host[:, 4 * BLOCK: 9 * BLOCK] = 32767
    d = torch.from_numpy(host).to(DEV)
    for cands, winner in (([160, 40], 160), ([40, 160], 40), ([40, 40, 160], 40)):
        rx = LiveReceiver(6, "auto", candidates=cands, max_burst_len=None, device=DEV)
        got = drive(rx, d, push_sizes(8192, host.shape[1]))
        rx.close()
        want = M.expected(host[0], cands)
        assert (want[0]["bit_frames"], want[0]["rate_score"], want[0]["clock_idx"]) == (winner, 32767, 0)
        for c in range(6):
            assert same(got[c], want), (cands, c)


def test_max_score_refuses_noise_bursts_and_decodes_the_message_behind_them(torch_cuda):
    torch = torch_cuda
    host, sent = M.noise_then_message_cases(M.SEED_NOISE)
    real, noise = M.score_gap(host, sent)
    assert real < noise
    limit = (real + noise) // 2
    rx = LiveReceiver(host.shape[0], "auto", max_score=limit, max_burst_len=None, progressive=True, device=DEV)
    assert rx.max_score == limit
    taps = []
    got = drive(rx, torch.from_numpy(host).to(DEV), push_sizes(8192, host.shape[1]),
                each=lambda out: taps.append((out.n_closed.cpu().numpy().copy(), out.tap.len.cpu().numpy().copy())))
    rx.close()
    for c in range(host.shape[0]):
        assert same(got[c], M.expected(host[c], None, limit)), c
        refused, message = got[c]
        assert (refused["status"], refused["nbytes"], refused["nbits"], refused["bit_frames"], refused["bytes"]) == \
            (_native.ST_INVALID_BAUD, 0, 0, 0, b"") and refused["rate_score"] > limit
        assert (refused["clock_idx"], refused["term_frame"]) == (-1, -1)
        assert (message["bit_frames"], message["bytes"], message["status"]) == (*sent[c], _native.ST_OK)
    # the refused bursts handed out no tap bytes: only the messages' 16 bytes per channel left the tap
    assert sum(int(tl[c, :nc[c]].sum()) for nc, tl in taps for c in range(host.shape[0])) <= 16 * host.shape[0]
    first = next((nc, tl) for nc, tl in taps if nc.any())
    assert all(tl[c, 0] == 0 for nc, tl in [first] for c in np.nonzero(nc)[0])


def test_a_short_burst_between_messages_reports_no_rate(torch_cuda):
    """A message, a one-block burst reported by a flush (TOO_SHORT, 0, -1), a message at another rate: the open burst's
    rate and score do not outlive the burst."""
    torch = torch_cuda
    rng = np.random.default_rng(6)
    n = 6
    sent = [[(M.RATES[c % 6], b"before the short"), (M.RATES[(c + 3) % 6], b"after the short!")] for c in range(n)]
    first = M.stack([M.rated_capture(rng, sent[c][:1]) for c in range(n)], BLOCK)
    first = np.concatenate([first, np.zeros((n, 2 * BLOCK), np.int16), np.full((n, BLOCK), 30000, np.int16)], axis=1)
    second = M.stack([M.rated_capture(rng, sent[c][1:]) for c in range(n)])
    rx = LiveReceiver(n, "auto", max_burst_len=None, device=DEV)
    got = drive(rx, torch.from_numpy(first).to(DEV), push_sizes(8192, first.shape[1]))
    more = drive(rx, torch.from_numpy(second).to(DEV), push_sizes(8192, second.shape[1]))
    rx.close()
    for c in range(n):
        assert same(got[c], M.expected(first[c])) and same(more[c], M.expected(second[c])), c
        a, short = got[c]
        assert (a["bit_frames"], a["bytes"]) == sent[c][0] and a["rate_score"] >= 0
        assert (short["status"], short["len"], short["flags"], short["bit_frames"], short["rate_score"]) == \
            (_native.ST_TOO_SHORT, BLOCK, _native.LIVE_OPEN_END, 0, -1)
        assert [(g["bit_frames"], g["bytes"]) for g in more[c]] == sent[c][1:]


# ------------------------------------------------------------------------------------------- graph, ragged, pairs


def test_graph_captured_push_matches_eager(torch_cuda, rate_case):
    torch = torch_cuda
    host, sent, want = rate_case
    n, T = host.shape[0], 2048
    total = -(-host.shape[1] // T) * T
    d = torch.zeros((n, total), dtype=torch.int16, device=DEV)
    d[:, : host.shape[1]] = torch.from_numpy(host).to(DEV)
    eager = LiveReceiver(n, "auto", max_burst_len=None, max_chunk_len=T, device=DEV)
    graphed = LiveReceiver(n, "auto", max_burst_len=None, max_chunk_len=T, device=DEV)
    src = torch.zeros((n, T), dtype=torch.int16, device=DEV)
    out_g = graphed.alloc_result(diagnostics=True)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graphed.push(src, out=out_g, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    graphed.reset()
    got_e, got_g = [[] for _ in range(n)], [[] for _ in range(n)]
    out_e = eager.alloc_result(diagnostics=True)
    for p in range(0, total, T):
        src.copy_(d[:, p: p + T])
        g.replay()
        collect(out_g, got_g, True)
        collect(eager.push(d[:, p: p + T], out=out_e), got_e, True)
    assert got_e == got_g
    check_rate_case(without_corrected(got_g), sent, want)
    torch.cuda.synchronize()
    eager.close()
    graphed.close()


def without_corrected(rows):
    return [[{k: v for k, v in g.items() if k != "corrected"} for g in ch] for ch in rows]


def test_ragged_ticks_a_masked_reset_and_masked_flushes(torch_cuda, rate_case):
    """Every channel takes its own number of samples per tick (device lengths, 0 included); half-way channels 1 and 4
    are reset; at the end the odd channels are flushed by a mask, then the even ones."""
    torch = torch_cuda
    host, sent, want = rate_case
    n, total = host.shape
    T = 8192
    rng = np.random.default_rng(8)
    d = torch.from_numpy(host).to(DEV)
    rx = LiveReceiver(n, "auto", max_burst_len=None, max_chunk_len=T, device=DEV)
    out = rx.alloc_result()
    got = [[] for _ in range(n)]
    pos = np.zeros(n, np.int64)
    buf = torch.full((n, T), 12345, dtype=torch.int16, device=DEV)       # (what lies beyond a length is loud garbage)
    lens_d = torch.zeros(n, dtype=torch.int32, device=DEV)
    cols = torch.arange(T, device=DEV)[None, :]
    reset_at, reset_mask = None, np.array([0, 1, 0, 0, 1, 0], np.uint8)

    def tick():
        lens = np.minimum(rng.choice([0, 1, 7, 2047, 2048, 2049, 5000, T], n), total - pos).astype(np.int32)
        idx = torch.from_numpy(pos).to(DEV)[:, None] + cols
        rows = torch.gather(d, 1, idx.clamp(max=total - 1))
        lens_d.copy_(torch.from_numpy(lens))
        buf.copy_(torch.where(cols < lens_d[:, None], rows, torch.full_like(rows, 12345)))
        collect(rx.push(buf, out=out, lengths=lens_d), got)
        unused_slots_are_clear(out)
        pos[:] += lens

    while pos.min() < total // 2:
        tick()
    reset_at = pos.copy()
    rx.reset(reset_mask)
    while pos.min() < total:
        tick()
    odd = np.arange(n) % 2 == 1
    collect(rx.flush(out=out, mask=odd), got)
    collect(rx.flush(out=out, mask=~odd), got)
    collect(rx.flush(out=out), got)                                       # (nothing is left to report)
    rx.close()
    for c in range(n):
        if reset_mask[c]:
            # what was reported before the reset, then a new stream from the reset on
            before = [w for w in want[c] if w["start"] + w["len"] <= reset_at[c]]
            assert same(got[c][: len(before)], before), c
            assert same(got[c][len(before):], M.expected(host[c, reset_at[c]:])), c
        else:
            assert same(got[c], want[c]), c


def test_a_threshold_pair_per_channel(torch_cuda):
    """Channels 1 and 4 at half scale with their own pair: the per-channel cells, the squelch from the channel's
    amp_end and the burst's rate."""
    torch = torch_cuda
    host, sent = M.rate_cases(M.SEED_THRESHOLDS, scale=M.HALF_SCALE)
    pairs = [M.HALF_PAIRS[s != 1.0] for s in M.HALF_SCALE]
    rx = LiveReceiver(6, "auto", [p[0] for p in pairs], [p[1] for p in pairs], max_burst_len=None, device=DEV)
    assert rx.amp_start_threshold is None and list(rx.channel_amp_end) == [p[1] for p in pairs]
    got = drive(rx, torch.from_numpy(host).to(DEV),
                push_sizes("random", host.shape[1], np.random.default_rng(9), STEPS))
    rx.close()
    check_rate_case(got, sent, [M.expected(cap, None, None, *pairs[c]) for c, cap in enumerate(host)])
    # at the full-scale pair the half-scale channels would not even open a burst
    assert M.expected(host[1]) == []


# --------------------------------------------------------------------------------- progressive, events, segments


@pytest.mark.parametrize("r", [40, 160])
def test_progressive_tap_arrays_equal_the_fixed_progressive_receivers(torch_cuda, r):
    torch = torch_cuda
    rng = np.random.default_rng(r)
    n = 6
    host = M.stack([M.rated_capture(rng, [(r, bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(2)])
                    for _ in range(n)])
    d = torch.from_numpy(host).to(DEV)
    sizes = push_sizes("random", host.shape[1], rng, STEPS)
    taps = {}
    for kind, bf, kw in (("fixed", r, {}), ("auto", "auto", dict(candidates=[r]))):
        rx = LiveReceiver(n, bf, max_burst_len=None, max_payload_len=0, progressive=True, device=DEV, **kw)
        rows = []

        def each(out):
            nn = out.tap.n.cpu().numpy()
            tb = out.tap.bytes.cpu().numpy()
            rows.append([tb[c, : nn[c]].tobytes() for c in range(n)]
                        + [getattr(out.tap, f).cpu().numpy().copy() for f in TAP_FIELDS[1:]])

        taps[kind] = (drive(rx, d, sizes, each=each), rows, rx.tap_cap)
        rx.close()
    assert taps["auto"][2] == taps["fixed"][2]
    assert without_rates(taps["auto"][0]) == taps["fixed"][0]
    for a, f in zip(taps["auto"][1], taps["fixed"][1]):
        assert a[:n] == f[:n]
        for x, y in zip(a[n:], f[n:]):
            assert np.array_equal(x, y)
    assert any(any(row[:n]) for row in taps["auto"][1])


def test_progressive_assembler_events_and_segments_with_all_candidates(torch_cuda, rate_case):
    torch = torch_cuda
    host, sent, want = rate_case
    n = host.shape[0]
    rx = LiveReceiver(n, "auto", max_burst_len=None, max_payload_len=0, progressive=True, device=DEV)
    asm_r, asm_s = rx.assembler(), rx.assembler()
    ev, sg = rx.alloc_events(), rx.alloc_segments()
    out = rx.alloc_result()
    d = torch.from_numpy(host).to(DEV)
    whole, whole_s, rated, p = [], [], [], 0
    for t in push_sizes(8192, host.shape[1]) + [0]:
        res = rx.push(d[:, p: p + t], out=out, flush=t == 0, events=ev, segments=sg)
        p += t
        assert res.events.bursts() == res.bursts()
        recs = res.events.records()
        bf = res.bit_frames.cpu().numpy()
        assert np.array_equal(res.events.bit_frames(), bf[recs["channel"], recs["slot"]])
        assert res.events.bit_frames().dtype == np.int32
        assert res.segments.partials() == res.partials()
        rb = res.rated_bursts()
        assert [b[:4] for b in rb] == res.bursts() and [b[4] for b in rb] == res.events.bit_frames().tolist()
        rated += rb
        whole += asm_r.feed(res)
        whole_s += asm_s.feed(res.segments)
    rx.close()
    assert whole == whole_s
    by_channel = [[(b[3]) for b in whole if b[0] == c] for c in range(n)]
    assert by_channel == [[p for _, p in sent[c]] for c in range(n)]      # whole payloads at max_payload_len = 0
    assert [[b[4] for b in rated if b[0] == c] for c in range(n)] == [[bf for bf, _ in sent[c]] for c in range(n)]
    assert [(b[1], b[2]) for b in rated if b[0] == 0] == [(w["start"], w["len"]) for w in want[0]]


def test_out_must_come_from_this_receivers_alloc_result(torch_cuda):
    torch = torch_cuda
    auto = LiveReceiver(2, "auto", max_burst_len=None, max_chunk_len=4096, device=DEV)
    fixed = LiveReceiver(2, 40, max_burst_len=None, max_chunk_len=4096, device=DEV)
    chunk = torch.zeros((2, 4096), dtype=torch.int16, device=DEV)
    res = fixed.alloc_result()
    assert res.bit_frames is None and res.rate_score is None and fixed.push(chunk, out=res).bit_frames is None
    with pytest.raises(ValueError, match="auto receiver"):
        auto.push(chunk, out=res)
    mine = auto.alloc_result()
    assert mine.bit_frames.dtype == torch.int32 and tuple(mine.rate_score.shape) == (2, auto.slots)
    auto.push(chunk, out=mine)
    with pytest.raises(ValueError, match="auto receiver"):
        fixed.push(chunk).rated_bursts()
    torch.cuda.synchronize()
    auto.close()
    fixed.close()
