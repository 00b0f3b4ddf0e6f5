"""GPU parity (-m gpu) of the packed event list (``afsk_live_pack``, ``LiveReceiver.push(events=)``, ``LiveEvents``).

Expected values never come from the pack kernels: hand-made slot arrays are packed by the numpy model
(tests/live_events_model.py), and real receivers are compared with the slot arrays of the same push (``collect``,
``LiveResult.bursts``) and, over a whole capture, with the CPU oracle's gate and demodulator over each channel's capture
(``want``).  Integer outputs: every comparison is exact."""
import functools

import numpy as np
import pytest

from afskmodem_amd import _native, live
from tests import live_events_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live import FIELDS, collect
from tests.test_gpu_live_ragged import T, channel, channels, extra, plan, receiver
from tests.test_gpu_live_tap import stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN = 256                                         # AFSK_LIVE_EVENTS_SPAN: the channels one block scans
FILL, MARKER = 0x5A, 0xEE


# ----------------------------------------------------------------------------------------- packing hand-made arrays

def device_pack(torch, arrays, max_events, max_bytes):
    """afsk_live_pack over hand-made arrays into an events buffer filled with FILL: the buffer on the host, with the
    offsets of its parts."""
    nc, start, length, flags, rows, demod = arrays
    n, slots = length.shape
    stride = rows.shape[1]
    ro, po, total = live.events_layout(n, slots, max_events, max_bytes)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    d = [t(a) for a in (nc, start, length, flags, rows)] + [t(demod[f]) for f in M.FIELDS]
    ev = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    _native.check(_native.lib().afsk_live_pack(
        n, slots, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
        d[4].data_ptr() if stride else None, stride, *(x.data_ptr() for x in d[5:]), ev.data_ptr(), max_events,
        max_bytes, None))
    torch.cuda.synchronize()
    return ev.cpu().numpy(), ro, po


def assert_packed(buf, ro, po, arrays, max_events, max_bytes, tag):
    """The header, the records and the payload bytes equal the model's, and nothing else of the record and payload
    parts was written."""
    h, recs, pay = M.pack(*arrays, max_events, max_bytes)
    assert (ro, po) == (32, 32 + 48 * max_events)
    got = buf[:32].view(M.HEADER)[0]
    assert got.tobytes() == h.tobytes(), (tag, got, h)
    assert buf[ro: ro + recs.nbytes].tobytes() == recs.tobytes(), tag
    assert (buf[ro + recs.nbytes: po] == FILL).all(), tag
    assert buf[po: po + len(pay)].tobytes() == pay, tag
    assert (buf[po + len(pay): po + max_bytes] == FILL).all(), tag
    assert MARKER not in pay, tag
    return h[0], recs


@pytest.mark.parametrize("n", [1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 7])
def test_hand_made_arrays_pack_as_the_model_packs_them(torch_cuda, n):
    rng = np.random.default_rng(100 + n)
    seen_overflow = seen_truncated = records = 0
    for slots in (1, 2, 3):
        for stride in (0, 12, 172, 384):
            for pattern in ("zero", "full", "sparse", "last", "first"):
                arrays = M.random_push(rng, n, slots, stride, pattern, MARKER)
                count = int(arrays[0].sum())
                if pattern == "full":
                    assert count == n * slots
                max_events, max_bytes = n * slots, n * slots * stride       # the capacities that never overflow
                buf, ro, po = device_pack(torch_cuda, arrays, max_events, max_bytes)
                h, recs = assert_packed(buf, ro, po, arrays, max_events, max_bytes, (slots, stride, pattern))
                assert h["count"] == h["stored"] == count and h["n_bytes"] == h["stored_bytes"]
                assert (recs["payload_offset"] >= 0).all()
                seen_overflow += int(np.count_nonzero(recs["flags"] & M.OVERFLOW))
                seen_truncated += int(np.count_nonzero(recs["nbytes"] > stride))
                records += count
    assert records > 0 and seen_overflow > 0 and seen_truncated > 0


def test_capacities_bound_what_is_written(torch_cuda):
    rng = np.random.default_rng(9)
    n, slots, stride = 2 * SPAN + 150, 2, 172
    arrays = M.random_push(rng, n, slots, stride, "sparse", MARKER)
    full, all_recs, pay = M.pack(*arrays, n * slots, n * slots * stride)
    count, kept = int(full["count"][0]), int(full["n_bytes"][0])
    assert count > 8 and kept > 400 and len({int(c) // SPAN for c in all_recs["channel"]}) == 3
    for max_events in (count - 1, count, count + 1):
        for max_bytes in (kept - 1, kept, kept + 1):
            buf, ro, po = device_pack(torch_cuda, arrays, max_events, max_bytes)
            h, recs = assert_packed(buf, ro, po, arrays, max_events, max_bytes, (max_events, max_bytes))
            assert (h["count"], h["n_bytes"]) == (count, kept)                  # the true totals
            assert h["stored"] == min(count, max_events) == recs.size
            off = np.concatenate([[0], np.cumsum(np.where(all_recs["flags"] & M.OVERFLOW, 0,
                                                          np.clip(all_recs["nbytes"], 0, stride)))])
            fits = off[1:] <= max_bytes
            assert np.array_equal(recs["payload_offset"], np.where(fits, off[:-1], -1)[: recs.size])
            assert h["stored_bytes"] == off[1:][: recs.size][fits[: recs.size]].max(initial=0)
    # a payload part that ends in the middle of the list: later records -1, an empty kept payload at the edge is not
    cut = int(all_recs["payload_offset"][count // 2])
    buf, ro, po = device_pack(torch_cuda, arrays, count, cut)
    h, recs = assert_packed(buf, ro, po, arrays, count, cut, "cut")
    assert h["stored_bytes"] <= cut and (recs["payload_offset"] == -1).any() and (recs["payload_offset"] >= 0).any()
    buf, ro, po = device_pack(torch_cuda, arrays, 0, 0)
    h, recs = assert_packed(buf, ro, po, arrays, 0, 0, "nothing")
    assert (h["count"], h["stored"], h["n_bytes"], h["stored_bytes"]) == (count, 0, kept, 0)


# ----------------------------------------------------------------------------------- real receivers against the oracle

@functools.lru_cache(maxsize=None)
def plain_plan():
    """The channels of ``channels("mixed_pairs")`` padded with silence to one length, a multiple of T: (channels with
    the oracle's bursts over the padded captures, push buffers [P, n, T])."""
    chans = channels("mixed_pairs")
    width = -(-max(len(ch["cap"]) for ch in chans) // T) * T
    host = np.zeros((len(chans), width), np.int16)
    for c, ch in enumerate(chans):
        host[c, : len(ch["cap"])] = ch["cap"]
    padded = tuple(channel(host[c], ch["bf"], ch["a_start"], ch["a_end"], ch["case"]) for c, ch in enumerate(chans))
    return padded, np.ascontiguousarray(host.reshape(len(chans), width // T, T).transpose(1, 0, 2))


def check_push(res, ev, acc):
    """One push: the packed list is the slot arrays' list, field for field; the bursts are added to acc[c]."""
    assert res.events is ev and ev.result is res
    bursts = ev.bursts()
    assert bursts == res.bursts()
    rows = [[] for _ in acc]
    collect(res, rows)
    flat = [(c, k, g) for c, got in enumerate(rows) for k, g in enumerate(got)]
    recs = ev.records()
    assert ev.count == len(flat) and recs.size == min(len(flat), ev.max_events)
    for i, r in enumerate(recs):
        c, k, g = flat[i]
        assert (int(r["channel"]), int(r["slot"])) == (c, k), i
        assert (int(r["burst_start"]), int(r["burst_len"]), int(r["flags"])) == (g["start"], g["len"], g["flags"]), i
        for f in FIELDS:
            assert int(r[f]) == g[f], (i, f)
        assert ev.payload(i) == g["bytes"], i
    for (c, k, g), b in zip(flat, bursts):
        assert b == (c, g["start"], g["len"], b"" if g["flags"] & _native.LIVE_OVERFLOW else g["bytes"])
        acc[c].append((g["start"], g["len"], g["flags"], b[3]))
    return recs


def check_capture(chans, acc):
    for c, ch in enumerate(chans):
        assert acc[c] == list(ch["want"]), c
    with_bursts = [c for c, ch in enumerate(chans) if ch["want"]]
    assert len(with_bursts) >= len(chans) - 2 and all(acc[c] for c in with_bursts)


def run_capture(torch, kind, form, ev_sizes=None):
    """A whole capture through push(events=ev): (channels, the bursts per channel, the records of every push)."""
    if form == "plain":
        chans, host = plain_plan()
        sched = [(None, None)] * host.shape[0]
    else:
        chans, sched, host = plan("mixed_pairs")
    rx = receiver(chans, kind)
    assert rx.slots == 2 and (rx.progressive, rx.streaming) == (kind == "tapped", kind != "stored")
    ev = rx.alloc_events(*ev_sizes) if ev_sizes else rx.alloc_events()
    dev = torch.from_numpy(host).to(DEV)
    acc, pushes = [[] for _ in chans], []
    for p, (lens, mask) in enumerate(sched):
        if form == "plain":
            res = rx.push(dev[p], flush=p == len(sched) - 1, events=ev)
        else:
            res = rx.push(dev[p], lengths=torch.from_numpy(lens).to(DEV) if p % 2 else lens,
                          flush=mask.astype(bool) if mask.any() else False, events=ev)
        recs = check_push(res, ev, acc)
        pushes.append((ev.header().copy(), recs))
    rx.close()
    return chans, acc, pushes


@pytest.mark.parametrize("form", ["plain", "ragged"])
@pytest.mark.parametrize("kind", ["stored", "stream", "tapped"])
def test_receivers_report_the_oracles_bursts_through_the_packed_list(torch_cuda, kind, form):
    chans, acc, pushes = run_capture(torch_cuda, kind, form)
    check_capture(chans, acc)
    assert all(h["count"] == h["stored"] and h["n_bytes"] == h["stored_bytes"] for h, _ in pushes)
    assert max(h["count"] for h, _ in pushes) >= 2 and min(h["count"] for h, _ in pushes) == 0
    assert not hasattr(receiver_push_without_events(torch_cuda, kind), "events")


def receiver_push_without_events(torch, kind):
    rx = receiver(channels("mixed_pairs"), kind)
    res = rx.push(torch.zeros((rx.n_channels, T), dtype=torch.int16, device=DEV))
    torch.cuda.synchronize()
    rx.close()
    return res


def test_small_capacities_still_give_complete_bursts(torch_cuda):
    chans, acc, pushes = run_capture(torch_cuda, "stored", "ragged", ev_sizes=(1, 6))
    check_capture(chans, acc)
    assert any(h["count"] > h["stored"] == 1 for h, _ in pushes)                     # records past max_events
    assert any(r.size and (r["payload_offset"] == -1).any() for _, r in pushes)      # payloads past max_bytes
    assert any(r.size and (r["payload_offset"] >= 0).all() and h["count"] == 1 for h, r in pushes)


# ------------------------------------------------------------------------------------------------------ graph capture

@functools.lru_cache(maxsize=None)
def graph_plan():
    """8 channels at 1200 and 300 baud; a 300-baud burst opens in one push and closes two pushes later."""
    chans = tuple(extra(40 + c, 40 if c % 2 == 0 else 160, nbytes=(5, 9) if c % 2 == 0 else (4, 5)) for c in range(8))
    host = stack([ch["cap"] for ch in chans])
    host = np.concatenate([host, np.zeros((8, -host.shape[1] % T), np.int16)], axis=1)
    spans = [(s // T, (s + n - 1) // T) for ch in chans for s, n, _, _ in ch["want"]]
    assert any(b - a >= 2 for a, b in spans)
    return chans, host


@pytest.mark.parametrize("kind", ["stored", "stream"])
def test_a_captured_push_and_pack_replays_like_the_eager_calls(torch_cuda, kind):
    torch = torch_cuda
    chans, host = graph_plan()
    dev = torch.from_numpy(host).to(DEV)
    pushes = host.shape[1] // T
    eager_rx = receiver(chans, kind)
    ev = eager_rx.alloc_events()
    eager = []
    for p in range(pushes):
        res = eager_rx.push(dev[:, p * T:(p + 1) * T], events=ev)
        eager.append((res.events.bursts(), ev.records().tobytes()))
    eager_rx.close()
    assert sum(len(b) for b, _ in eager) == sum(len(ch["want"]) for ch in chans) > 8

    rx = receiver(chans, kind)
    buf = torch.zeros((8, T), dtype=torch.int16, device=DEV)
    res, ev = rx.alloc_result(), rx.alloc_events()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rx.push(buf, out=res, events=ev, stream=side)          # a linear chain: the push's launches, then the pack's
    torch.cuda.synchronize()
    got = [[] for _ in chans]
    for p in range(pushes):
        buf.copy_(dev[:, p * T:(p + 1) * T])
        graph.replay()
        assert (ev.bursts(), ev.records().tobytes()) == eager[p], p
        assert ev.bursts() == res.bursts(), p
        for c, s, n, data in ev.bursts():
            got[c].append((s, n, data))
    for c, ch in enumerate(chans):
        assert got[c] == [(w[0], w[1], w[3]) for w in ch["want"]], c      # (padded with silence: nothing stays open)
    rx.close()
