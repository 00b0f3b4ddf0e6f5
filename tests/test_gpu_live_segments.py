"""GPU parity (-m gpu) of the packed segment list (``afsk_live_pack_tap``, ``LiveReceiver.push(segments=)``,
``LiveSegments``, ``PayloadAssembler.feed(LiveSegments)``).

Expected values never come from the pack kernels: hand-made tap arrays are packed by the numpy model
(tests/live_segments_model.py), and progressive receivers are compared with the tap arrays of the same push
(``LiveResult.partials``) and, over a whole capture, with the CPU oracle's gate and demodulator over each channel's
capture (``want``).  Integer outputs: every comparison is exact."""
import functools

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_segments_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live_events import graph_plan, plain_plan
from tests.test_gpu_live_ragged import T, channel, channels, plan, receiver
from tests.test_gpu_live_tap import BLOCK, expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN = 256                                         # AFSK_LIVE_EVENTS_SPAN: the channels one block scans
FILL, MARKER = 0x5A, 0xEE


# ----------------------------------------------------------------------------------------- packing hand-made arrays

def device_pack(torch, arrays, max_segments, max_bytes):
    """afsk_live_pack_tap over hand-made arrays into a segments buffer filled with FILL: the buffer on the host, with
    the offsets of its parts."""
    n, slots = arrays[7].shape
    cap = arrays[5].shape[1]
    ro, do, total = live.segments_layout(n, slots, max_segments, max_bytes)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    sg = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    _native.check(_native.lib().afsk_live_pack_tap(n, slots, cap, *(x.data_ptr() for x in d), sg.data_ptr(),
                                                   max_segments, max_bytes, None))
    torch.cuda.synchronize()
    return sg.cpu().numpy(), ro, do


def assert_packed(buf, ro, do, arrays, max_segments, max_bytes, tag):
    """The header, the records and the data bytes equal the model's, and nothing else of the record and data parts was
    written."""
    h, recs, data = M.pack(arrays, max_segments, max_bytes)
    assert (ro, do) == (32, 32 + 32 * max_segments)
    got = buf[:32].view(M.HEADER)[0]
    assert got.tobytes() == h.tobytes(), (tag, got, h)
    assert buf[ro: ro + recs.nbytes].tobytes() == recs.tobytes(), tag
    assert (buf[ro + recs.nbytes: do] == FILL).all(), tag
    assert buf[do: do + len(data)].tobytes() == data, tag
    assert (buf[do + len(data): do + max_bytes] == FILL).all(), tag
    assert MARKER not in data, tag
    return h[0], recs


@pytest.mark.parametrize("n", [1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 7])
def test_hand_made_arrays_pack_as_the_model_packs_them(torch_cuda, n):
    rng = np.random.default_rng(200 + n)
    seen = dict(records=0, empty_final=0, open=0, orphan=0, clamped=0)
    for slots in (1, 2, 3):
        for cap in (1, 8, 19, 183):
            for pattern in M.PATTERNS:
                arrays = M.random_tap(rng, n, slots, cap, pattern, MARKER)
                max_segments, max_bytes = n * (slots + 1), n * cap           # the capacities that never overflow
                buf, ro, do = device_pack(torch_cuda, arrays, max_segments, max_bytes)
                h, recs = assert_packed(buf, ro, do, arrays, max_segments, max_bytes, (slots, cap, pattern))
                assert h["count"] == h["stored"] == recs.size and h["n_bytes"] == h["stored_bytes"]
                nc, tap_n, open_start = arrays[0], arrays[6], arrays[8]
                if pattern == "nothing":
                    assert h["count"] == 0 and h["n_bytes"] == 0
                elif pattern == "open_only":
                    assert h["count"] == n and (recs["slot"] == -1).all() and h["n_bytes"] == tap_n.sum()
                elif pattern == "all":
                    assert np.count_nonzero(recs["slot"] >= 0) == n * slots and h["n_bytes"] == n * cap
                elif pattern == "span_last":
                    assert set(recs["channel"].tolist()) <= set(range(SPAN - 1, n, SPAN)) | {n - 1}
                elif pattern == "orphan":
                    seen["orphan"] += int(np.count_nonzero((open_start == -1) & (tap_n > 0)))
                    assert h["n_bytes"] <= tap_n.sum()
                elif pattern == "wild":
                    seen["clamped"] += int(np.count_nonzero((nc > slots) | (nc < 0) | (tap_n > cap) | (tap_n < 0)))
                seen["records"] += int(h["count"])
                seen["empty_final"] += int(np.count_nonzero((recs["slot"] >= 0) & (recs["length"] == 0)))
                seen["open"] += int(np.count_nonzero(recs["slot"] == -1))
    assert all(v > 0 for k, v in seen.items() if n >= 63 or k in ("records", "open")), seen


def test_capacities_bound_what_is_written(torch_cuda):
    rng = np.random.default_rng(9)
    n, slots, cap = 2 * SPAN + 150, 2, 19
    arrays = M.random_tap(rng, n, slots, cap, "random", MARKER)
    segs = M.segments(*arrays)
    count, nb = len(segs), sum(len(d) for _, d in segs)
    assert count > 100 and nb > 400 and len({r[0] // SPAN for r, _ in segs}) == 3
    for max_segments in (count - 1, count, count + 1):
        for max_bytes in (nb - 1, nb, nb + 1):
            buf, ro, do = device_pack(torch_cuda, arrays, max_segments, max_bytes)
            h, recs = assert_packed(buf, ro, do, arrays, max_segments, max_bytes, (max_segments, max_bytes))
            assert (h["count"], h["n_bytes"]) == (count, nb)                    # the true totals
            assert h["stored"] == min(count, max_segments) == recs.size
            if max_segments >= count and max_bytes >= nb:
                assert h["stored_bytes"] == nb
    # a data part that ends inside ONE channel's run: a final segment of the channel is written, its next one is not
    off = 0
    for i, (r, d) in enumerate(segs):
        nxt = segs[i + 1] if i + 1 < count else None
        if i > count // 2 and r[1] >= 0 and len(d) > 0 and nxt and nxt[0][0] == r[0] and len(nxt[1]) > 1:
            cut = off + len(d) + 1
            break
        off += len(d)
    else:
        raise AssertionError("no channel with two segments that hold bytes")
    buf, ro, do = device_pack(torch_cuda, arrays, count, cut)
    h, recs = assert_packed(buf, ro, do, arrays, count, cut, "straddle")
    assert h["stored_bytes"] == cut - 1 and h["stored"] == count
    # records that end inside one channel's run, with room for every byte
    buf, ro, do = device_pack(torch_cuda, arrays, i + 1, nb)
    h, recs = assert_packed(buf, ro, do, arrays, i + 1, nb, "records straddle")
    assert h["stored_bytes"] == cut - 1 and recs["channel"][-1] == segs[i + 1][0][0]
    buf, ro, do = device_pack(torch_cuda, arrays, 0, 0)
    h, recs = assert_packed(buf, ro, do, arrays, 0, 0, "nothing")
    assert (h["count"], h["stored"], h["n_bytes"], h["stored_bytes"]) == (count, 0, nb, 0)


# --------------------------------------------------------------------------- progressive receivers against the oracle

@functools.lru_cache(maxsize=None)
def capture_plan(form):
    """(channels, schedule, push buffers [P, n, T], the channel to reset, the push before which it is reset, its stream
    position then): the existing small plans -- ``mixed_pairs`` padded to whole pushes, or under its ragged schedule
    -- and a reset of the channel with the longest payload, at least four blocks into that burst (bytes of it have
    arrived by then) and more than a block before its end."""
    if form == "plain":
        chans, host = plain_plan()
        sched = [(None, None)] * host.shape[0]
    else:
        chans, sched, host = plan("mixed_pairs")
    rc, j = max(((c, j) for c, ch in enumerate(chans) for j in range(len(ch["want"]))),
                key=lambda cj: len(chans[cj[0]]["want"][cj[1]][3]))
    if form == "plain":
        consumed = [T * p for p in range(len(sched))]
    else:
        consumed = np.concatenate([[0], np.cumsum([int(lens[rc]) for lens, _ in sched])]).tolist()
    s0, n0 = chans[rc]["want"][j][:2]
    reset_at = next(p for p in range(len(sched)) if consumed[p] >= s0 + 4 * BLOCK)
    assert consumed[reset_at] < s0 + n0 - BLOCK and len(chans[rc]["want"][j][3]) >= 100
    return chans, sched, host, rc, reset_at, consumed[reset_at]


def run_capture(torch, form, sizes=None):
    """A whole capture through push(segments=sg) of a progressive receiver, with ``events=`` on every other push:
    after every push the packed list is the result's own ``partials()``; one assembler is fed the segments, one the
    results.  One channel is reset in the middle of its first burst (``capture_plan``; both assemblers learn of it
    from open_start alone).  Returns (the two assemblers' bursts, headers per push)."""
    chans, sched, host, rc, reset_at, _ = capture_plan(form)
    sched = list(sched)
    rx = receiver(chans, "tapped")
    assert rx.slots == 2 and rx.progressive
    sg = rx.alloc_segments(*sizes) if sizes else rx.alloc_segments()
    ev = rx.alloc_events()
    dev = torch.from_numpy(host).to(DEV)
    by_segments, by_results = rx.assembler(), rx.assembler()
    got_s, got_r, headers = [], [], []
    mask = np.zeros(len(chans), np.uint8)
    mask[rc] = 1
    held = False
    for p, (lens, fmask) in enumerate(sched):
        if p == reset_at:
            held = rc in by_segments.pending()
            rx.reset(mask)
        kw = dict(segments=sg, events=ev if p % 2 else None)
        if form == "plain":
            res = rx.push(dev[p], flush=p == len(sched) - 1, **kw)
        else:
            res = rx.push(dev[p], lengths=torch.from_numpy(lens).to(DEV) if p % 2 else lens,
                          flush=fmask.astype(bool) if fmask.any() else False, **kw)
        assert res.segments is sg and sg.result is res and hasattr(res, "events") == bool(p % 2)
        want = res.partials()
        assert sg.partials() == want, p
        h = sg.header().copy()
        assert h["count"] == len(want) and h["n_bytes"] == sum(len(w[3]) for w in want)
        if p % 2:
            assert ev.bursts() == res.bursts()
        headers.append(h)
        got_s += by_segments.feed(sg)
        got_r += by_results.feed(res)
        assert by_segments.pending() == by_results.pending(), p
    rx.close()
    assert got_s == got_r and by_segments.pending() == {}
    return got_s, headers, held


def check_capture(form, got):
    """The assembled bursts are the oracle's with their whole payloads; the channel that was reset in mid-burst reports
    what the oracle gates in the rest of its capture, a new stream."""
    chans, _, _, rc, _, reset_pos = capture_plan(form)
    for c, ch in enumerate(chans):
        want = ch["want"]
        if c == rc:
            want = [w for w in want if w[0] + w[1] <= reset_pos] + \
                expected(ch["cap"][reset_pos:], ch["bf"], ch["a_start"], ch["a_end"])
        assert [b[1:] for b in got if b[0] == c] == [(w[0], w[1], w[3]) for w in want], c
    assert sum(1 for b in got if b[3]) >= len(chans) // 2


@pytest.mark.parametrize("form", ["plain", "ragged"])
def test_progressive_receivers_report_the_oracles_payloads_through_the_packed_list(torch_cuda, form):
    got, headers, held = run_capture(torch_cuda, form)
    assert len({ch["bf"] for ch in capture_plan(form)[0]}) > 1                     # mixed rates
    check_capture(form, got)
    assert held                                          # the reset dropped a burst the assemblers held bytes of
    assert all(h["count"] == h["stored"] and h["n_bytes"] == h["stored_bytes"] for h in headers)
    assert max(h["count"] for h in headers) >= 2 and min(h["count"] for h in headers) == 0


def test_one_rate_receiver_through_the_packed_list(torch_cuda):
    torch = torch_cuda
    chans = channels("uniform")
    width = -(-max(len(ch["cap"]) for ch in chans) // T) * T
    host = np.zeros((len(chans), width), np.int16)
    for c, ch in enumerate(chans):
        host[c, : len(ch["cap"])] = ch["cap"]
    chans = [channel(host[c], ch["bf"], ch["a_start"], ch["a_end"]) for c, ch in enumerate(chans)]     # (padded)
    rx = receiver(chans, "tapped")
    assert rx.bit_frames == 40
    sg, asm, dev, got = rx.alloc_segments(), rx.assembler(), torch.from_numpy(host).to(DEV), []
    for p in range(width // T):
        res = rx.push(dev[:, p * T:(p + 1) * T], segments=sg)
        assert sg.partials() == res.partials(), p
        got += asm.feed(sg)
    got += asm.feed(rx.flush(segments=sg).segments)
    for c, ch in enumerate(chans):
        assert [b[1:] for b in got if b[0] == c] == [(w[0], w[1], w[3]) for w in ch["want"]], c
    rx.close()


@pytest.mark.parametrize("sizes", [(1, 4096), (64, 3), (0, 0)])
def test_small_capacities_fall_back_to_the_tap_arrays(torch_cuda, sizes):
    got, headers, _ = run_capture(torch_cuda, "ragged", sizes=sizes)
    check_capture("ragged", got)
    assert any(h["count"] > h["stored"] or h["n_bytes"] > h["stored_bytes"] for h in headers)
    assert all(h["stored"] <= sizes[0] and h["stored_bytes"] <= sizes[1] for h in headers)


def test_segments_on_a_receiver_that_is_not_progressive_raise(torch_cuda):
    torch = torch_cuda
    chans = channels("mixed_pairs")
    tapped = receiver(chans, "tapped")
    sg = tapped.alloc_segments()
    chunk = torch.zeros((len(chans), T), dtype=torch.int16, device=DEV)
    for kind in ("stored", "stream"):
        rx = receiver(chans, kind)
        with pytest.raises(ValueError):
            rx.push(chunk, segments=sg)
        with pytest.raises(ValueError):
            rx.flush(segments=sg)
        with pytest.raises(ValueError):
            rx.alloc_segments()
        res = rx.push(chunk)
        with pytest.raises(ValueError):
            rx.pack_tap(res, out=sg)
        assert not hasattr(res, "segments")
        rx.close()
    res = tapped.push(chunk)
    assert not hasattr(res, "segments") and not hasattr(res, "events")
    assert tapped.pack_tap(res).partials() == []                                   # a fresh buffer of the default size
    torch.cuda.synchronize()
    tapped.close()


# ------------------------------------------------------------------------------------------------------ graph capture

def test_a_captured_push_and_pack_replays_like_the_eager_calls(torch_cuda):
    torch = torch_cuda
    chans, host = graph_plan()
    dev = torch.from_numpy(host).to(DEV)
    pushes = host.shape[1] // T
    eager_rx = receiver(chans, "tapped")
    sg = eager_rx.alloc_segments()

    def parts(sg):
        """The header and the records, and the data bytes, as the buffer holds them."""
        h = sg.header()
        buf = sg.buffer.cpu().numpy()
        return (buf[: 32 + 32 * int(h["stored"])].tobytes(),
                buf[sg.data_offset: sg.data_offset + int(h["stored_bytes"])].tobytes())

    eager = []
    for p in range(pushes):
        res = eager_rx.push(dev[:, p * T:(p + 1) * T], segments=sg)
        eager.append((res.partials(), *parts(sg)))
    eager_rx.close()
    assert sum(len(e[0]) for e in eager) > 16 and any(not f for e in eager for *_, f in e[0])

    rx = receiver(chans, "tapped")
    src = torch.zeros((len(chans), T), dtype=torch.int16, device=DEV)
    res, sg = rx.alloc_result(), rx.alloc_segments()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rx.push(src, out=res, segments=sg, stream=side)       # a linear chain: the push's launch, then the pack's
    torch.cuda.synchronize()
    rx.reset()
    asm, got = rx.assembler(), []
    for p in range(pushes):
        src.copy_(dev[:, p * T:(p + 1) * T])
        graph.replay()
        assert (sg.partials(), *parts(sg)) == eager[p], p
        assert sg.partials() == res.partials(), p
        got += asm.feed(sg)
    for c, ch in enumerate(chans):
        assert [b[1:] for b in got if b[0] == c] == [(w[0], w[1], w[3]) for w in ch["want"]], c
    rx.close()
