"""GPU parity (-m gpu) of the two packers -- ``afsk_live_pack`` and ``afsk_live_pack_tap`` -- where their launches take
paths the smaller tests never reach: more than 65536 channels (the one-block scan of the span totals then takes a
second and a third step, with a carry between them), capacities that cut the list past the first step, payload rows
wide enough for a lane's second 16-byte store at every alignment, and byte totals past 2^31 and 2^32.

Expected values never come from a pack kernel: hand-made arrays are packed by the vectorised numpy models
(``pack_fast`` of tests/live_events_model.py and tests/live_segments_model.py, which the host tests hold equal to the
models' plain loops), and real receivers are compared with the slot and tap arrays of the same push.  Integer outputs:
every comparison is exact."""
import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from afskmodem_amd.live import LiveReceiver
from tests import live_events_model as EM
from tests import live_segments_model as SM
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live_events import assert_packed as assert_packed_events
from tests.test_gpu_live_events import check_push
from tests.test_gpu_live_events import device_pack as pack_events
from tests.test_gpu_live_segments import assert_packed as assert_packed_segments
from tests.test_gpu_live_segments import device_pack as pack_segments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN = 256                                         # AFSK_LIVE_EVENTS_SPAN: the channels one block scans
STEP = SPAN * SPAN                                 # the channels one step of the scan kernel covers: 65536
FILL, MARKER = 0x5A, 0xEE
SIZES = (STEP, STEP + 1, 2 * STEP + 300)           # 256, 257 and 513 scratch entries: 1, 2 and 3 steps
SLOTS, STRIDE, CAP = 2, 12, 19
PATTERNS = ("full", "sparse", "wild", "last", "second_step_only", "first_step_only")


# ------------------------------------------------------------------------------------------- hand-made large pushes

def joined(parts):
    """The pushes ``parts`` as one push over their channels in order (every array of both models is channel-major)."""
    if isinstance(parts[0][5], dict):
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(5)) + \
            ({f: np.concatenate([p[5][f] for p in parts]) for f in EM.FIELDS},)
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(SM.NAMES)))


def large_push(kind, n, pattern, seed):
    """Hand-made arrays of ``n`` channels for the events (``kind`` "events") or the segments packer.  ``pattern``, in
    the events / segments model's words: "full" / "all"; "sparse" / "random"; "wild"; "last" (the very last channel
    alone); "second_step_only" (nothing below channel 65536); "first_step_only" (nothing from it on).  Every part that
    reports at all ends in a channel that reports all its slots, so that the last channel before 65536, and the last
    of all, are never silent by chance."""
    rng = np.random.default_rng(seed)
    if kind == "events":
        make = lambda m, p: EM.random_push(rng, m, SLOTS, STRIDE, p, MARKER)  # noqa: E731
        names = dict(full="full", some="sparse", wild="wild", none="zero")
    else:
        make = lambda m, p: SM.random_tap(rng, m, SLOTS, CAP, p, MARKER)  # noqa: E731
        names = dict(full="all", some="random", wild="wild", none="nothing")

    def busy(m, p):
        return [(m - 1, names[p]), (1, names["full"])]

    plan = {"full": [(n, names["full"])], "sparse": busy(n, "some"), "wild": busy(n, "wild"),
            "last": [(n - 1, names["none"]), (1, names["full"])],
            "second_step_only": [(STEP, names["none"])] + (busy(n - STEP, "some") if n > STEP else []),
            "first_step_only": busy(STEP, "some") + [(n - STEP, names["none"])]}[pattern]
    arrays = joined([make(m, p) for m, p in plan if m > 0])
    assert arrays[0].shape == (n,)
    return arrays


def events_model(arrays, max_events, max_bytes):
    """(header, records, payload bytes) of the events model's ``pack_fast``."""
    h, recs, copies = EM.pack_fast(*arrays, max_events, max_bytes)
    return h, recs, EM.gather(arrays[4], copies)


def segments_model(arrays, max_segments, max_bytes):
    h, recs, copies = SM.pack_fast(arrays, max_segments, max_bytes)
    return h, recs, SM.gather(arrays[5], copies)


def assert_buffer(buf, ro, po, model, max_records, max_bytes, tag):
    """The header, the records and the bytes equal the model's, and everything else of the record and byte parts still
    holds FILL."""
    h, recs, data = model
    assert (ro, po) == (32, 32 + recs.dtype.itemsize * max_records)
    got = buf[:32].view(EM.HEADER)[0]
    assert got.tobytes() == h.tobytes(), (tag, got, h)
    got_recs = buf[ro: ro + recs.nbytes].view(recs.dtype)
    for f in recs.dtype.names:
        bad = np.nonzero(got_recs[f] != recs[f])[0]
        assert bad.size == 0, (tag, f, bad.size, int(bad[0]), got_recs[bad[0]], recs[bad[0]])
    assert (buf[ro + recs.nbytes: po] == FILL).all(), tag
    got_data = buf[po: po + len(data)]
    bad = np.nonzero(got_data != np.frombuffer(data, np.uint8))[0]
    assert bad.size == 0, (tag, "bytes", bad.size, int(bad[0]))
    assert (buf[po + len(data): po + max_bytes] == FILL).all(), tag
    assert int(h["stored_bytes"][0]) == len(data) and MARKER not in data, tag
    return h[0], recs


def check_sides(n, pattern, recs):
    """From the model alone: the records lie on the side(s) of channel 65536 the pattern promises."""
    below, above = bool((recs["channel"] < STEP).any()), bool((recs["channel"] >= STEP).any())
    if pattern == "second_step_only":
        assert not below and above == (n > STEP)
    elif pattern == "first_step_only":
        assert below and not above
    elif pattern == "last":
        assert set(recs["channel"].tolist()) == {n - 1}
    else:
        assert below and above == (n > STEP)
        if n > 2 * STEP:
            assert (recs["channel"] >= 2 * STEP).any()                # the third step's channels too


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_events_pack_over_more_than_one_scan_step(torch_cuda, n, pattern):
    arrays = large_push("events", n, pattern, 300 + n % 1000)
    max_events, max_bytes = n * SLOTS, n * SLOTS * STRIDE               # the capacities that never overflow
    model = events_model(arrays, max_events, max_bytes)
    check_sides(n, pattern, model[1])
    if pattern == "full":
        assert model[1].size == n * SLOTS
    if pattern == "wild":
        nc = arrays[0]
        assert (nc < 0).sum() > 100 and (nc > SLOTS).sum() > 100 and model[0]["count"][0] == np.clip(nc, 0, SLOTS).sum()
    buf, ro, po = pack_events(torch_cuda, arrays, max_events, max_bytes)
    h, recs = assert_buffer(buf, ro, po, model, max_events, max_bytes, (n, pattern))
    assert h["count"] == h["stored"] == recs.size and h["n_bytes"] == h["stored_bytes"]
    assert (recs["payload_offset"] >= 0).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_segments_pack_over_more_than_one_scan_step(torch_cuda, n, pattern):
    arrays = large_push("segments", n, pattern, 400 + n % 1000)
    max_segments, max_bytes = n * (SLOTS + 1), n * CAP                  # the capacities that never overflow
    model = segments_model(arrays, max_segments, max_bytes)
    check_sides(n, pattern, model[1])
    if pattern == "full":
        assert np.count_nonzero(model[1]["slot"] >= 0) == n * SLOTS and model[0]["n_bytes"][0] == n * CAP
    if pattern == "wild":
        nc, tn = arrays[0], arrays[6]
        assert min((nc < 0).sum(), (nc > SLOTS).sum(), (tn < 0).sum(), (tn > CAP).sum()) > 100
    buf, ro, do = pack_segments(torch_cuda, arrays, max_segments, max_bytes)
    h, recs = assert_buffer(buf, ro, do, model, max_segments, max_bytes, (n, pattern))
    assert h["count"] == h["stored"] == recs.size and h["n_bytes"] == h["stored_bytes"]


# ------------------------------------------------------------------------- capacities that cut past the first scan step

def first_left_out(lengths, max_records, max_bytes):
    """W: the index of the first record that is left out or whose bytes are, from the full list's byte lengths."""
    over = np.nonzero(np.cumsum(lengths) > max_bytes)[0]
    return min(max_records, int(over[0]) if over.size else len(lengths))


def cuts(all_recs, lengths):
    """(name, max_records, max_bytes) of the cuts: by the record capacity alone, by the byte capacity alone, and by both
    -- the bytes first, and the records first -- each at a record of the second or the third scan step."""
    count, nb = all_recs.size, int(lengths.sum())
    end = np.cumsum(lengths)
    chan = all_recs["channel"]
    in2 = int(np.nonzero((chan >= STEP + 1000) & (lengths > 0))[0][0])          # a record of the second step
    in3 = int(np.nonzero((chan >= 2 * STEP + 10) & (lengths > 0))[0][0])        # and one of the third, with bytes
    assert chan[in2] < 2 * STEP <= chan[in3]
    return [("records", in3, nb, in3), ("bytes", count, int(end[in2]) - 1, in2),
            ("bytes_then_records", in3, int(end[in2]) - 1, in2), ("records_then_bytes", in2, int(end[in3]) - 1, in2)]


@pytest.mark.parametrize("cut", ["records", "bytes", "bytes_then_records", "records_then_bytes"])
def test_events_capacities_cut_past_the_first_scan_step(torch_cuda, cut):
    n = SIZES[2]
    arrays = large_push("events", n, "sparse", 500)
    _, all_recs, copies = EM.pack_fast(*arrays, n * SLOTS, n * SLOTS * STRIDE)
    lengths = copies[:, 2]
    name, max_events, max_bytes, w = next(c for c in cuts(all_recs, lengths) if c[0] == cut)
    assert first_left_out(lengths, max_events, max_bytes) == w and all_recs["channel"][w] >= STEP
    model = events_model(arrays, max_events, max_bytes)
    h, recs, _ = model
    assert (h["count"][0], h["n_bytes"][0]) == (all_recs.size, lengths.sum())       # the true totals
    assert h["stored"][0] == max_events == recs.size and h["stored_bytes"][0] == lengths[:w].sum()
    if cut in ("bytes", "bytes_then_records"):
        assert (recs["payload_offset"][w:] == -1).all() and recs.size > w and (recs["payload_offset"][:w] >= 0).all()
    buf, ro, po = pack_events(torch_cuda, arrays, max_events, max_bytes)
    assert_buffer(buf, ro, po, model, max_events, max_bytes, cut)


@pytest.mark.parametrize("cut", ["records", "bytes", "bytes_then_records", "records_then_bytes"])
def test_segments_capacities_cut_past_the_first_scan_step(torch_cuda, cut):
    n = SIZES[2]
    arrays = large_push("segments", n, "sparse", 600)
    _, all_recs, _ = SM.pack_fast(arrays, n * (SLOTS + 1), n * CAP)
    lengths = all_recs["length"].astype(np.int64)
    name, max_segments, max_bytes, w = next(c for c in cuts(all_recs, lengths) if c[0] == cut)
    assert first_left_out(lengths, max_segments, max_bytes) == w and all_recs["channel"][w] >= STEP
    model = segments_model(arrays, max_segments, max_bytes)
    h, recs, _ = model
    assert (h["count"][0], h["n_bytes"][0]) == (all_recs.size, lengths.sum())       # the true totals
    assert h["stored"][0] == max_segments == recs.size and h["stored_bytes"][0] == lengths[:w].sum()
    buf, ro, do = pack_segments(torch_cuda, arrays, max_segments, max_bytes)
    assert_buffer(buf, ro, do, model, max_segments, max_bytes, cut)


# -------------------------------------------------------------------------------- wide rows, every alignment of a copy

@pytest.mark.parametrize("stride", [1040, 2049, 65536])
def test_wide_rows_copy_at_every_alignment(torch_cuda, stride):
    """``live_events_copy`` moves a payload as a head up to the destination's 16-byte boundary, 16-byte stores -- a lane
    takes a second one from 1024 body bytes on -- and a tail.  Pushes of 70 channels are packed until, by the model
    alone, the payloads of more than 1024 kept bytes have started at every destination offset mod 16 and the kept
    lengths have taken every value mod 16.  (At stride 1040 few records keep more than 1024 bytes: more pushes.)"""
    n, slots = 70, 2
    rng = np.random.default_rng(700 + stride)
    starts, tails, second_round, flagged = set(), set(), set(), 0
    for push in range(64):
        arrays = EM.random_push(rng, n, slots, stride, "full", MARKER, uniform=True)
        max_events, max_bytes = n * slots, n * slots * stride            # the capacities that never overflow
        model = events_model(arrays, max_events, max_bytes)
        _, recs, copies = EM.pack_fast(*arrays, max_events, max_bytes)
        kept, off = copies[:, 2], copies[:, 3]
        assert (off == recs["payload_offset"]).all() and (off >= 0).all()
        starts |= set((off[kept > 1024] % 16).tolist())
        tails |= set((kept[kept > 0] % 16).tolist())
        # the copies in which a lane does store twice: 1040 bytes or more behind the head
        second_round |= set((off[kept - (-off) % 16 >= 1040] % 16).tolist())
        flagged += int(np.count_nonzero(recs["flags"] & EM.OVERFLOW))
        buf, ro, po = pack_events(torch_cuda, arrays, max_events, max_bytes)
        h, _ = assert_buffer(buf, ro, po, model, max_events, max_bytes, (stride, push))
        assert_packed_events(buf, ro, po, arrays, max_events, max_bytes, (stride, push))     # (the plain model too)
        assert h["count"] == h["stored"] == n * slots and h["n_bytes"] == h["stored_bytes"]
        if len(starts) == 16 and len(tails) == 16 and (len(second_round) == 16 or stride == 1040):
            break
    assert starts == set(range(16)) and tails == set(range(16)) and flagged > 0, (push, starts, tails)
    # (the 1040 kept bytes of the narrowest rows give a second round only behind an empty head)
    assert second_round <= {0} if stride == 1040 else second_round == set(range(16))


def test_tap_rows_filled_to_a_wide_cap(torch_cuda):
    n, slots, cap = 70, 2, 4096
    arrays = SM.random_tap(np.random.default_rng(8), n, slots, cap, "all", MARKER)
    assert (arrays[6] == cap).all()
    max_segments, max_bytes = n * (slots + 1), n * cap
    model = segments_model(arrays, max_segments, max_bytes)
    assert model[0]["count"][0] == max_segments and model[0]["n_bytes"][0] == max_bytes
    buf, ro, do = pack_segments(torch_cuda, arrays, max_segments, max_bytes)
    assert_buffer(buf, ro, do, model, max_segments, max_bytes, "wide cap")
    assert_packed_segments(buf, ro, do, arrays, max_segments, max_bytes, "wide cap")      # (the plain model too)


# --------------------------------------------------------------------------------- byte totals past 2^31 and 2^32

def need_memory(torch):
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("needs ~9 GB of free HBM")


def random_rows(torch, n, width):
    """uint8 [n, width] of random bytes, made on the device."""
    rows = torch.empty((n, width), dtype=torch.uint8, device=DEV)
    for lo in range(0, n, 8192):
        hi = min(lo + 8192, n)
        rows[lo:hi] = torch.randint(0, 256, (hi - lo, width), dtype=torch.uint8, device=DEV)
    return rows


def assert_device_buffer(torch, buf, ro, po, model, rows, max_records, max_bytes, tag):
    """``assert_buffer`` for a byte part too large for the host: header and records on the host, against the model;
    the written bytes -- by the model's copy list the first W rows' leading bytes, back to back -- and the FILL behind
    them on the device."""
    h, recs, copies = model
    assert (ro, po) == (32, 32 + recs.dtype.itemsize * max_records)
    head = buf[:po].cpu().numpy()
    got = head[:32].view(EM.HEADER)[0]
    assert got.tobytes() == h.tobytes(), (tag, got, h)
    assert head[ro: ro + recs.nbytes].tobytes() == recs.tobytes(), tag
    assert (head[ro + recs.nbytes:] == FILL).all(), tag
    w = int(np.count_nonzero(copies[:, 2] > 0))
    width = int(copies[0, 2])
    assert np.array_equal(copies[:w], np.stack([np.arange(w), np.zeros(w, np.int64), np.full(w, width),
                                                np.arange(w) * width], axis=1)) and (copies[w:, 2] == 0).all()
    assert int(h["stored_bytes"][0]) == w * width <= max_bytes
    part = buf[po: po + max_bytes]
    assert torch.equal(part[: w * width].view(w, width), rows[:w, :width]), tag
    assert bool((part[w * width:] == FILL).all()), tag


def test_events_byte_totals_past_2_32(torch_cuda):
    torch = torch_cuda
    need_memory(torch)
    n, slots, stride = STEP + 1, 1, 65536
    nc = np.ones(n, np.int32)
    rng = np.random.default_rng(12)
    start = (rng.integers(0, 1 << 40, (n, slots)) * 2048).astype(np.int64)
    length = (rng.integers(1, 64, (n, slots)) * 2048).astype(np.int32)
    flags = rng.choice([0, 1], (n, slots)).astype(np.int32)                     # (no OVERFLOW)
    demod = {f: rng.integers(-50, 1 << 20, n * slots).astype(np.int32) for f in EM.FIELDS}
    demod["nbytes"][:] = stride
    full, _, _ = EM.pack_fast(nc, start, length, flags, stride, demod, n, 2 ** 31 - 1)
    assert full["count"][0] == n and full["n_bytes"][0] == 2 ** 32 + 65536       # (also a second scan step)
    rows = random_rows(torch, n * slots, stride)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    d = [t(a) for a in (nc, start, length, flags)] + [t(demod[f]) for f in EM.FIELDS]
    for max_events, max_bytes, written in ((5, 3 * 65536 + 100, 3), (n, 2 ** 31 - 1, 32767)):
        model = EM.pack_fast(nc, start, length, flags, stride, demod, max_events, max_bytes)
        h, recs, _ = model
        assert (h["count"][0], h["stored"][0], h["n_bytes"][0]) == (n, max_events, 2 ** 32 + 65536)
        assert h["stored_bytes"][0] == written * 65536
        assert recs["payload_offset"].tolist() == [i * 65536 if i < written else -1 for i in range(max_events)]
        ro, po, total = live.events_layout(n, slots, max_events, max_bytes)
        ev = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
        _native.check(_native.lib().afsk_live_pack(
            n, slots, *(x.data_ptr() for x in d[:4]), rows.data_ptr(), stride, *(x.data_ptr() for x in d[4:]),
            ev.data_ptr(), max_events, max_bytes, None))
        torch.cuda.synchronize()
        assert_device_buffer(torch, ev, ro, po, model, rows, max_events, max_bytes, (max_events, max_bytes))
        del ev


def test_segments_byte_totals_past_2_31(torch_cuda):
    torch = torch_cuda
    need_memory(torch)
    n, slots, cap = STEP + 1, 1, 40000
    rng = np.random.default_rng(13)
    z = np.zeros((n, slots), np.int32)
    arrays = [np.zeros(n, np.int32), z.astype(np.int64), z, z, np.zeros(n * slots, np.int32), cap,
              np.full(n, cap, np.int32), z, (rng.integers(0, 1 << 40, n) * 2048).astype(np.int64),
              (cap + rng.integers(0, 1 << 16, n)).astype(np.int32)]
    max_segments, max_bytes = 5, 100000
    model = SM.pack_fast(arrays, max_segments, max_bytes)
    h, recs, _ = model
    assert (h["count"][0], h["stored"][0], h["n_bytes"][0], h["stored_bytes"][0]) == (n, 5, n * cap, 2 * cap)
    assert n * cap > 2 ** 31 and (recs["slot"] == -1).all() and (recs["length"] == cap).all()
    rows = random_rows(torch, n, cap)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if i != 5 else rows for i, a in enumerate(arrays)]
    ro, do, total = live.segments_layout(n, slots, max_segments, max_bytes)
    sg = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    _native.check(_native.lib().afsk_live_pack_tap(n, slots, cap, *(x.data_ptr() for x in d), sg.data_ptr(),
                                                   max_segments, max_bytes, None))
    torch.cuda.synchronize()
    assert_device_buffer(torch, sg, ro, do, model, rows, max_segments, max_bytes, "segments")


# -------------------------------------------------------------------------------- real receivers past 65536 channels

N_LIVE, T = STEP + SPAN + 1, 8192                  # 258 spans: a second scan step of two entries
BURSTS = (0, 255, 65535, 65536, 65791, 65792)      # the ends of the first, the 256th, the 257th and the 258th span
LEAD = 1000


def live_capture(torch):
    """(payload per burst channel, their waveforms [6, L] on the device behind LEAD samples of silence, L a multiple of
    T with room for the gate to close)."""
    pays = {c: bytes([c & 255, c >> 8 & 255, c >> 16, 0xA5]) for c in BURSTS}
    assert len(set(pays.values())) == len(BURSTS)
    tr = afskmodem.Transmitter(1200, 0.05)
    waves = [np.asarray(tr.wav_samples(pays[c]), np.int16) for c in BURSTS]
    width = -(-(LEAD + max(w.size for w in waves) + 4 * 2048) // T) * T
    host = np.zeros((len(BURSTS), width), np.int16)
    for i, w in enumerate(waves):
        host[i, LEAD: LEAD + w.size] = w
    return pays, torch.from_numpy(host).to(DEV)


def live_pushes(torch, waves):
    """The capture in chunks of T as [N_LIVE, T] device buffers, then chunks of silence: every channel but BURSTS is
    silent throughout."""
    rows = torch.as_tensor(BURSTS, device=DEV)
    buf = torch.zeros((N_LIVE, T), dtype=torch.int16, device=DEV)
    for p in range(waves.shape[1] // T + 4):
        buf[rows] = waves[:, p * T:(p + 1) * T] if (p + 1) * T <= waves.shape[1] else 0
        yield buf


def test_a_streaming_receiver_past_65536_channels_reports_through_the_packed_list(torch_cuda):
    torch = torch_cuda
    pays, waves = live_capture(torch)
    rx = LiveReceiver(N_LIVE, 40, max_burst_len=None, max_payload_len=8, max_chunk_len=T, device=DEV)
    ev = rx.alloc_events()
    assert (ev.max_events, ev.max_bytes) == (N_LIVE * rx.slots, N_LIVE * rx.slots * 8)
    ro, po, total = live.events_layout(N_LIVE, rx.slots, ev.max_events, ev.max_bytes)
    assert int(ev.buffer.numel()) == total == (po + ev.max_bytes + 15) // 16 * 16 + 16 * 258
    acc, counts = [[] for _ in range(N_LIVE)], []
    for chunk in live_pushes(torch, waves):
        check_push(rx.push(chunk, events=ev), ev, acc)
        counts.append(ev.count)
        if sum(counts) >= len(BURSTS):
            break
    rx.close()
    assert sum(counts) == len(BURSTS) and max(counts) > 1
    assert [c for c in range(N_LIVE) if acc[c]] == list(BURSTS)                      # all other channels: nothing
    for c in BURSTS:
        assert [b[3] for b in acc[c]] == [pays[c]], c


def test_a_progressive_receiver_past_65536_channels_reports_through_the_packed_list(torch_cuda):
    torch = torch_cuda
    pays, waves = live_capture(torch)
    rx = LiveReceiver(N_LIVE, 40, max_burst_len=None, max_payload_len=0, max_chunk_len=T, device=DEV, progressive=True)
    sg = rx.alloc_segments()
    assert (sg.max_segments, sg.max_bytes) == (N_LIVE * (rx.slots + 1), N_LIVE * rx.tap_cap)
    ro, do, total = live.segments_layout(N_LIVE, rx.slots, sg.max_segments, sg.max_bytes)
    assert int(sg.buffer.numel()) == total == (do + sg.max_bytes + 15) // 16 * 16 + 16 * 258
    by_segments, by_results = rx.assembler(), rx.assembler()
    got, segments = [], 0
    for p, chunk in enumerate(live_pushes(torch, waves)):
        res = rx.push(chunk, segments=sg)
        assert res.segments is sg and sg.result is res
        want = res.partials()
        assert sg.partials() == want, p
        h = sg.header()
        assert h["count"] == h["stored"] == len(want) and h["n_bytes"] == h["stored_bytes"] == sum(len(w[3]) for w in want)
        assert {w[0] for w in want} <= set(BURSTS)                                   # all other channels: nothing
        segments += len(want)
        new = by_segments.feed(sg)
        assert new == by_results.feed(res) and by_segments.pending() == by_results.pending(), p
        got += new
        if len(got) >= len(BURSTS):
            break
    rx.close()
    assert by_segments.pending() == {} and segments >= len(BURSTS)
    assert sorted((b[0], b[3]) for b in got) == [(c, pays[c]) for c in BURSTS]
