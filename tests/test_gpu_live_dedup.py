"""GPU parity (-m gpu) of the duplicate filter (``afsk_live_dedup_*``, ``LiveDedup``) and of the relay with a verdict per
record (``afsk_live_tx_submit_events_kept``, ``LiveTransmitter.submit_events(keep=)``).

Expected values never come from the kernels under test.  Hand-written event buffers are decided by the model
(tests/live_dedup_model.py): the verdicts are compared entry by entry and the table afterwards byte for byte, with poison
behind the verdicts and in every ring the call must not touch.  ``keep`` of all ones is held against the relay without
``keep`` on a twin transmitter, ``keep`` with zeros against the relay model.  Real audio and the chain A - B - C on a
``LiveMedium`` are judged by what goes on air.  Integer outputs and samples: every comparison is exact."""
import numpy as np
import pytest

from afskmodem_amd import _native, live
from afskmodem_amd.live import LiveDedup, LiveMedium, LiveReceiver, LiveTransmitter
from tests import live_dedup_model as D
from tests import live_events_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.test_gpu_live_relay import (BAUD, assert_outputs, assert_pulls, device_events, hand_cases, model_of,
                                       model_relay, preload)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x6B6B6B6B
W = 1000                                                 # the hand-written lists' window, in samples
OK, NO_DATA = _native.ST_OK, _native.ST_NO_DATA
Q, NONE = _native.LIVE_TX_QUEUED, _native.LIVE_TX_NONE
LENS = (1, 15, 16, 17, 63, 64, 65, 255, 256)
COUNTS = (0, 1, 3, 4, 5, 16, 17)                         # the per-wave (4) and per-block (16) edges


def odd_blob(pays):
    """The payloads back to back, each behind a pad where needed so that it starts at an ODD offset."""
    blob, offs = bytearray(), []
    for p in pays:
        if len(blob) % 2 == 0:
            blob.append(0xEE)
        offs.append(len(blob))
        blob += p
    return offs, bytes(blob)


def rows_of(items):
    """Event rows and the payload part of ``items`` -- (channel, payload, end time) each."""
    offs, blob = odd_blob([p for _, p, _ in items])
    return [(ch, t - 2048, 2048, 0, OK, len(p), off) for (ch, p, t), off in zip(items, offs)], blob


def poisoned(torch, n_channels, depth, seed, window=W):
    """A filter and its model whose rings hold random entries and heads: what a call must leave alone is visible."""
    rng = np.random.default_rng(seed)
    model = D.DedupModel(n_channels, depth)
    model.entries["key"] = rng.integers(0, 2 ** 63, (n_channels, depth)).astype(np.uint64) * 2 + 1
    model.entries["time"] = rng.integers(-5, 5, (n_channels, depth))
    model.entries["time"][rng.random((n_channels, depth)) < 0.3] = D.EMPTY
    model.head[:] = rng.integers(0, depth, n_channels)
    dd = LiveDedup(n_channels, depth=depth, window=window, device=DEV)
    dd.load_state(model.entries, model.head)
    return dd, model


def same_state(dd, model, tag):
    entries, head = dd.state()
    assert entries.dtype == live.DEDUP_STATE_DTYPE and entries.tobytes() == model.entries.tobytes(), tag
    assert (head == model.head).all(), tag


def check(torch, dd, model, buf, me, mb, stride, tag, window=None, skip=None):
    """One filter of the host buffer ``buf`` on ``dd`` against ``model``: the verdicts, the poison behind them, the table
    afterwards and the events buffer.  Returns the verdicts."""
    ev, whole = device_events(torch, buf, model.n, 1, stride, me, mb)
    big = torch.full((me + 8,), POISON, dtype=torch.int32, device=DEV)
    kw = {} if skip is None else dict(skip_flags=skip)
    out = dd.filter(ev, out=big[:me], window=window, **kw)
    want = model.filter(buf, me, mb, stride, dd.window if window is None else window,
                        D.OPEN_END if skip is None else skip)
    got = big.cpu().numpy()
    assert out.data_ptr() == big.data_ptr()
    assert (got[:me] == want).all(), (tag, got[:me].tolist(), want.tolist())
    assert (got[me:] == POISON).all(), tag
    assert (ev.buffer.cpu().numpy() == whole).all(), tag             # nothing of the events buffer is written
    same_state(dd, model, tag)
    return want


# --------------------------------------------------------------------------------------------- hand-written lists

@pytest.mark.parametrize("depth", [1, 8, 64])
def test_record_counts_payload_lengths_and_both_window_edges(torch_cuda, depth):
    """One record per channel, 0 ... 17 of them, every payload length at an odd offset: new; again W - 1 samples later: a
    duplicate (which refreshes nothing); again W samples after the first: new."""
    torch = torch_cuda
    rng = np.random.default_rng(depth)
    dd, model = poisoned(torch, 20, depth, 100 + depth)
    for n in COUNTS:
        pays = [bytes(rng.integers(0, 256, LENS[(i + n) % len(LENS)], dtype=np.uint8)) for i in range(n)]
        t0 = 10000 * (n + 1)
        for shift, verdict in ((0, D.NEW), (W - 1, D.DUP), (W, D.NEW)):
            rows, blob = rows_of([(i + 1, p, t0 + i + shift) for i, p in enumerate(pays)])
            assert all(r[6] % 2 == 1 for r in rows)
            me, mb = n + 3, len(blob) + 5
            want = check(torch, dd, model, D.events_buffer(rows, me, mb, blob), me, mb, 256, (depth, n, shift))
            assert want.tolist() == [verdict] * n + [D.NONE] * 3
    assert {len(p) for p in pays} == set(LENS)
    torch.cuda.synchronize()
    dd.close()


@pytest.mark.parametrize("depth", [1, 8, 64])
def test_runs_that_cross_a_waves_indices_and_fill_the_ring(torch_cuda, depth):
    torch = torch_cuda
    dd, model = poisoned(torch, 8, depth, 200 + depth)
    a, b, c, d = b"alpha", b"bravo!", b"c", bytes(range(70))
    distinct = [bytes([i % 251, i // 251, 7]) for i in range(depth + 1)]
    items = [(0, a, 100)]
    items += [(2, p, 101 + i) for i, p in enumerate((a, b, a, c, b, d))]          # indices 1 ... 6: two waves' indices
    items += [(3, a, 110)]
    items += [(5, p, 120 + i) for i, p in enumerate(distinct + [distinct[0], distinct[-1]])]
    items += [(7, a, 130), (7, a, 130)]
    rows, blob = rows_of(items)
    me, mb = len(rows) + 1, len(blob)
    want = check(torch, dd, model, D.events_buffer(rows, me, mb, blob), me, mb, 128, depth).tolist()
    assert want[0] == D.NEW and want[7] == D.NEW and want[-3:] == [D.NEW, D.DUP, D.NONE]
    if depth >= 4:
        assert want[1:7] == [D.NEW, D.NEW, D.DUP, D.NEW, D.DUP, D.NEW]
    else:
        assert want[1:7] == [D.NEW] * 6                                             # one entry: a, b, a never meet
    at = 8 + depth + 1
    assert want[8:at] == [D.NEW] * (depth + 1) and want[at] == D.NEW               # the first one was pushed out
    assert want[at + 1] == (D.DUP if depth > 1 else D.NEW)
    torch.cuda.synchronize()
    dd.close()


def test_ineligible_records_channels_out_of_range_and_a_future_entry(torch_cuda):
    torch = torch_cuda
    dd, model = poisoned(torch, 2, 2, 7)
    rows, blob = rows_of([(0, b"seen", 3000)])
    check(torch, dd, model, D.events_buffer(rows, 1, len(blob), blob), 1, len(blob), 8, "seen")
    before = model.copy()
    pay = b"\xeeseen" + bytes(59)
    rows = [(-1, 0, 3020, 0, OK, 4, 1), (0, 0, 3020, 0, NO_DATA, 4, 1), (0, 0, 3020, 0, OK, 0, 1),
            (0, 0, 3020, 0, OK, 9, 1), (0, 0, 3020, 0, OK, 4, -1), (0, 0, 3020, 0, OK, 4, 61),
            (0, 0, 3020, D.OVERFLOW, OK, 4, 1), (0, 0, 3020, D.OPEN_END, OK, 4, 1), (2, 0, 3020, 0, OK, 4, 1),
            (2 ** 31 - 1, 0, 3020, 0, OK, 4, 1)]
    buf = D.events_buffer(rows, len(rows), 64, pay)
    assert check(torch, dd, model, buf, len(rows), 64, 8, "ineligible").tolist() == [D.PASS] * len(rows)
    assert model.entries.tobytes() == before.entries.tobytes()
    for skip in (0, D.OVERFLOW):
        want = check(torch, dd, model, buf, len(rows), 64, 8, ("skip", skip), skip=skip).tolist()
        assert want == [D.PASS] * 7 + [D.DUP] + [D.PASS] * 2
    # the stream restarted: the entry lies in the future, which is no duplicate
    rows, blob = rows_of([(0, b"seen", 2999)])
    assert check(torch, dd, model, D.events_buffer(rows, 1, len(blob), blob), 1, len(blob), 8, "future").tolist() == [D.NEW]
    # window 0 remembers and drops nothing
    rows, blob = rows_of([(1, b"w0", 50), (1, b"w0", 50)])
    assert check(torch, dd, model, D.events_buffer(rows, 2, len(blob), blob), 2, len(blob), 8, "w0", window=0).tolist() \
        == [D.NEW, D.NEW]
    torch.cuda.synchronize()
    dd.close()


def test_an_unsorted_tail_and_a_stored_count_beyond_the_list(torch_cuda):
    torch = torch_cuda
    dd, model = poisoned(torch, 6, 4, 11)
    items = [(0, b"a", 1), (2, b"b", 2), (2, b"b", 3), (1, b"c", 4), (3, b"a", 5), (3, b"a", 6)]
    rows, blob = rows_of(items)
    want = check(torch, dd, model, D.events_buffer(rows, 8, len(blob), blob), 8, len(blob), 8, "unsorted").tolist()
    assert want == [D.NEW, D.NEW, D.DUP, D.PASS, D.PASS, D.PASS, D.NONE, D.NONE]
    rows, blob = rows_of([(0, b"x", 10), (1, b"y", 11), (4, b"z", 12)])
    for me, stored, verdicts in ((2, 77, [D.NEW, D.NEW]), (3, 2 ** 31 - 1, [D.DUP, D.DUP, D.NEW]),
                                 (5, 2, [D.DUP, D.DUP, D.NONE, D.NONE, D.NONE]), (3, -4, [D.NONE] * 3),
                                 (3, 0, [D.NONE] * 3)):
        buf = D.events_buffer(rows, me, len(blob), blob, stored=stored)
        assert check(torch, dd, model, buf, me, len(blob), 8, ("stored", me, stored)).tolist() == verdicts
    torch.cuda.synchronize()
    dd.close()


# ------------------------------------------------------------------------------------------------ state across calls

def test_three_filters_a_masked_reset_and_a_note_carry_state(torch_cuda):
    torch = torch_cuda
    dd, model = poisoned(torch, 5, 3, 21, window=5000)
    pays = [b"one", b"two", b"three", b"four"]
    for k in range(3):                                       # every list repeats the one before and adds a payload
        rows, blob = rows_of([(c, p, 1000 * (k + 1) + c) for c in (0, 2, 4) for p in pays[: k + 2]])
        want = check(torch, dd, model, D.events_buffer(rows, len(rows), len(blob), blob), len(rows), len(blob), 8, k)
        per = [D.NEW] * 2 if k == 0 else [D.DUP] * (k + 1) + [D.NEW]
        assert want.tolist() == per * 3, k
    # depth 3 and four payloads: "one" was pushed out by "four"
    rows, blob = rows_of([(0, b"one", 4000), (0, b"two", 4001)])
    assert check(torch, dd, model, D.events_buffer(rows, 2, len(blob), blob), 2, len(blob), 8, "evicted").tolist() == \
        [D.NEW, D.NEW]
    mask = [False, False, True, False, False]
    dd.reset(mask)
    model.reset(mask)
    same_state(dd, model, "masked reset")
    rows, blob = rows_of([(2, b"four", 4100), (4, b"four", 4100)])
    assert check(torch, dd, model, D.events_buffer(rows, 2, len(blob), blob), 2, len(blob), 8, "after reset").tolist() == \
        [D.NEW, D.DUP]
    # note: host lists in any order, a channel outside the filter's, an empty message
    chans, msgs, times = [3, 1, 9, 1, 3, 0], [b"mine", b"mine", b"mine", b"mine", b"", b"x" * 40], [4200] * 6
    got = dd.note(chans, msgs, times).cpu().numpy()
    want = model.note_any_order(chans, msgs, times, 5000)
    assert (got == want).all() and want.tolist() == [D.NEW, D.NEW, D.PASS, D.DUP, D.PASS, D.NEW]
    same_state(dd, model, "note")
    rows, blob = rows_of([(1, b"mine", 4300), (3, b"mine", 4300), (4, b"mine", 4300)])
    assert check(torch, dd, model, D.events_buffer(rows, 3, len(blob), blob), 3, len(blob), 8, "noted").tolist() == \
        [D.DUP, D.DUP, D.NEW]
    # note: device tensors in place, a time tensor, lengths, a descending channel, poison behind the verdicts
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(DEV)  # noqa: E731
    mat = np.zeros((5, 6), np.uint8)
    dev_msgs = [b"mine", b"dev", b"dev", b"late", b"z"]
    for i, p in enumerate(dev_msgs):
        mat[i, : len(p)] = np.frombuffer(p, np.uint8)
    chans = [0, 2, 2, 1, 4]
    big = torch.full((5 + 4,), POISON, dtype=torch.int32, device=DEV)
    dd.note(t(chans, np.int32), t(mat, np.uint8), t([4400] * 5, np.int64), out=big[:5],
            lengths=t([len(p) for p in dev_msgs], np.int32))
    want = model.note(chans, dev_msgs, [4400] * 5, 5000, payload_stride=6)
    assert want.tolist() == [D.NEW, D.NEW, D.DUP, D.PASS, D.PASS]
    assert big.cpu().numpy().tolist() == want.tolist() + [POISON] * 4
    same_state(dd, model, "device note")
    dd.reset()
    model.reset()
    same_state(dd, model, "reset")
    assert (model.entries["time"] == D.EMPTY).all() and not model.head.any()
    torch.cuda.synchronize()
    dd.close()


def test_70000_channels_with_one_record_each(torch_cuda):
    torch = torch_cuda
    n, depth, t = 70000, 2, 50000
    rng = np.random.default_rng(70)
    pay = rng.integers(0, 256, (n, 6), dtype=np.uint8)
    model = D.DedupModel(n, depth)
    model.head[:] = rng.integers(0, depth, n)
    model.entries["key"][::2, 1] = D.keys_np(pay)[::2]       # every second channel heard its payload 10 samples ago,
    model.entries["time"][::2, 1] = t - 10
    model.entries["time"][::4, 1] = t - W                   # every fourth one W samples ago
    dd = LiveDedup(n, depth=depth, window=W, device=DEV)
    dd.load_state(model.entries, model.head)
    recs = np.zeros(n, M.EVENT)
    recs["channel"], recs["burst_start"], recs["burst_len"] = np.arange(n), t - 2048, 2048
    recs["nbytes"], recs["nbits"], recs["payload_offset"] = 6, 48, 6 * np.arange(n)
    want = check(torch, dd, model, D.events_buffer(recs, n, 6 * n, pay.tobytes()), n, 6 * n, 6, "70000")
    assert (want[2::4] == D.DUP).all() and (want[0::4] == D.NEW).all() and (want[1::2] == D.NEW).all()
    torch.cuda.synchronize()
    dd.close()


# ------------------------------------------------------------------------------------------ submit_events(keep=)

def transmitter(kind, case):
    kw = dict(queue_depth=case["depth"], max_payload_len=case["max_payload"], device=DEV)
    if kind == "uniform":
        return LiveTransmitter(case["n_tx"], BAUD, 0.0, **kw)
    if kind == "mixed":
        return LiveTransmitter(case["n_tx"], [(12000, 2400, 1200)[c % 3] for c in range(case["n_tx"])], 0.0, **kw)
    return LiveTransmitter(case["n_tx"], training_time=0.0, rates=[12000, 2400], **kw)


@pytest.mark.parametrize("kind", ["uniform", "mixed", "rated"])
def test_keep_of_all_ones_is_submit_events_bit_for_bit(torch_cuda, kind):
    torch = torch_cuda
    seen = set()
    for case in hand_cases(65)[::2]:
        buf, me, mb, want = model_relay(case, model_of(case))
        ev, whole = device_events(torch, buf, 65, case["slots"], case["stride"], me, mb)
        kw = dict(channel_map=None if case["cmap"] is None else case["cmap"].tolist(), skip_flags=case["skip"])
        if kind == "rated":
            rng = np.random.default_rng(me)
            ev.result.bit_frames = torch.from_numpy(rng.choice([4, 20, 0], (65, case["slots"])).astype(np.int32)).to(DEV)
            kw["rate"] = "heard"
        tx, twin = transmitter(kind, case), transmitter(kind, case)
        if case["preload"]:
            for x in (tx, twin):
                x.submit(*preload(case))
                x.pull(5000)
        ones = torch.ones(me, dtype=torch.int32, device=DEV)
        ones[1::3] = 2                                       # any value but 0 keeps
        ones[2::5] = -1
        got = tx.submit_events(ev, keep=ones, **kw).cpu()
        ref = twin.submit_events(ev, **kw).cpu()
        for g, w, name in zip(got, ref, ("status", "start", "n_samples")):
            assert (g == w).all(), (kind, case["tag"], name)
        seen |= set(got[0].tolist())
        for T in (2048, 6000):
            assert torch.equal(tx.pull(T), twin.pull(T)), (kind, case["tag"], T)
            assert torch.equal(tx.pending, twin.pending), (kind, case["tag"], T)
        assert (ev.buffer.cpu().numpy() == whole).all()
        torch.cuda.synchronize()
        tx.close()
        twin.close()
    assert {Q, _native.LIVE_TX_SKIPPED, NONE} <= seen and _native.LIVE_TX_DUPLICATE not in seen
    assert kind != "rated" or _native.LIVE_TX_BAD_RATE in seen


def test_keep_with_zeros_answers_duplicate_and_queues_the_rest_as_the_model_does(torch_cuda):
    torch = torch_cuda
    seen = set()
    for case in hand_cases(64) + hand_cases(300)[:6]:
        n_rx = case["n_rx"]
        buf, me, mb, _ = model_relay(case, model_of(case))
        rng = np.random.default_rng(me + 3)
        keep = rng.integers(0, 3, me).astype(np.int32)
        model = model_of(case)
        want = D.relay_kept(model, buf, me, mb, case["stride"], n_rx, keep, case["cmap"], case["skip"])
        plain = model_relay(case, model_of(case))[3]
        assert set(want[0][(want[0] != plain[0])].tolist()) <= {D.DUPLICATE, Q, _native.LIVE_TX_QUEUE_FULL}
        ev, whole = device_events(torch, buf, n_rx, case["slots"], case["stride"], me, mb)
        tx = LiveTransmitter(case["n_tx"], BAUD, 0.0, queue_depth=case["depth"], max_payload_len=case["max_payload"],
                             device=DEV)
        if case["preload"]:
            tx.submit(*preload(case))
            tx.pull(5000)
        res = tx.submit_events(ev, channel_map=None if case["cmap"] is None else case["cmap"].tolist(),
                               skip_flags=case["skip"], keep=torch.from_numpy(keep).to(DEV))
        assert_outputs(res, want, case["tag"])
        assert (ev.buffer.cpu().numpy() == whole).all(), case["tag"]
        assert_pulls(torch, tx, model, None, case["tag"])
        seen |= set(want[0].tolist())
        torch.cuda.synchronize()
        tx.close()
    assert {D.DUPLICATE, Q, _native.LIVE_TX_SKIPPED, _native.LIVE_TX_BAD_CHANNEL, NONE} <= seen


def test_python_refusals_launch_nothing(torch_cuda):
    torch = torch_cuda
    rows, blob = rows_of([(0, b"abc", 100), (1, b"abc", 100)])
    buf = D.events_buffer(rows, 4, 16, blob)
    ev, whole = device_events(torch, buf, 4, 1, 8, 4, 16)
    dd, model = poisoned(torch, 4, 2, 5)
    tx = LiveTransmitter(4, BAUD, 0.0, queue_depth=2, max_payload_len=8, device=DEV)
    keep = dd.alloc_verdict(4)
    assert keep.tolist() == [D.NONE] * 4
    with pytest.raises(TypeError):
        dd.filter(ev.buffer)
    with pytest.raises(ValueError):
        dd.filter(live.LiveEvents(whole, 4, 16, result=ev.result))               # a host buffer
    with pytest.raises(ValueError):
        dd.filter(live.LiveEvents(ev.buffer, 4, 16))                             # no result
    with pytest.raises(ValueError):
        dd.filter(ev, out=dd.alloc_verdict(5))
    with pytest.raises(TypeError):
        dd.filter(ev, out=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        dd.filter(ev, out=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        tx.submit_events(ev, keep=[1, 1, 1, 1])
    with pytest.raises(TypeError):
        tx.submit_events(ev, keep=torch.ones(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        tx.submit_events(ev, keep=torch.ones(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        tx.submit_events(ev, keep=torch.ones(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        dd.load_state(model.entries[:3], model.head)
    bad_head = model.head.copy()
    bad_head[1] = 2
    with pytest.raises(_native.AfskNativeError):
        dd.load_state(model.entries, bad_head)
    with pytest.raises(ValueError):
        dd.note(torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros((3, 4), dtype=torch.uint8, device=DEV),
                torch.zeros(3, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert keep.tolist() == [D.NONE] * 4 and (tx.pending == 0).all().item()
    same_state(dd, model, "refusals")
    assert (ev.buffer.cpu().numpy() == whole).all()
    rx = LiveReceiver(3, 40, max_burst_len=None, max_chunk_len=2048, max_payload_len=16, device=DEV)
    mine = rx.deduper(depth=5, window=2.0)
    assert (mine.n_channels, mine.depth, mine.window, mine.device) == (3, 5, 96000, rx.device)
    for x in (dd, tx, rx, mine):
        x.close()


# ------------------------------------------------------------------------------------------------------ real audio

CHUNK = 8192


def heard_twice(torch, window):
    """One payload sent twice into a streaming receiver at 1200 baud, the second copy 1.3 s behind the first one's end;
    the statuses of the two records a relay with a filter of ``window`` answers, in order."""
    kw = dict(queue_depth=4, max_payload_len=16, device=DEV)
    src, tx = LiveTransmitter(1, 1200, 0.05, **kw), LiveTransmitter(1, 1200, 0.05, **kw)
    rx = LiveReceiver(1, 40, max_burst_len=None, max_chunk_len=CHUNK, max_payload_len=16, device=DEV)
    dd = rx.deduper(depth=4, window=window)
    ev = rx.alloc_events()
    keep, sub = dd.alloc_verdict(ev.max_events), tx.alloc_submit_result(ev.max_events)
    statuses, verdicts, starts = [], [], []
    for t in range(24):
        if t in (0, 9):
            st, start, ns = src.submit([0], [b"twice!"]).cpu()
            assert st[0] == Q and start[0] == t * CHUNK
            starts.append(int(start[0] + ns[0]))
        rx.push(src.pull(CHUNK), events=ev)
        dd.filter(ev, out=keep)
        tx.submit_events(ev, keep=keep, out=sub)
        tx.pull(CHUNK)
        assert ev.bursts() == [] or ev.bursts()[0][3] == b"twice!"
        statuses += [int(s) for s in sub.status.cpu().numpy() if s != NONE]
        verdicts += [int(v) for v in keep.cpu().numpy() if v != D.NONE]
    assert starts[1] - starts[0] == 9 * CHUNK and 9 * CHUNK - (starts[0]) > 48000       # more than 1 s of silence between
    torch.cuda.synchronize()
    for x in (src, tx, rx, dd):
        x.close()
    return statuses, verdicts


def test_a_payload_heard_twice_is_relayed_once(torch_cuda):
    assert heard_twice(torch_cuda, 30.0) == ([Q, D.DUPLICATE], [D.NEW, D.DUP])


def test_a_window_shorter_than_the_gap_relays_both(torch_cuda):
    assert 48000 < 9 * CHUNK
    assert heard_twice(torch_cuda, 1.0) == ([Q, Q], [D.NEW, D.NEW])


# ------------------------------------------------------------------------------------- the chain A - B - C

P, T = 4, 2048
PAYS = [bytes([65 + c, 104, 97, 105, 110, 48 + c]) for c in range(P)]
GAIN = [[0, 1.0, 0], [1.0, 0, 1.0], [0, 1.0, 0]]          # A and C do not hear each other
TICKS = 40
NAMES = ("status", "start", "n_samples", "keep", "busy", "pending", "on_air")


class Station:
    def __init__(self, torch, rows, seed, dedup):
        self.rx = LiveReceiver(P, 40, max_burst_len=None, max_chunk_len=T, max_payload_len=16, device=DEV)
        self.tx = LiveTransmitter(P, 1200, 0.05, queue_depth=4, max_payload_len=16, device=DEV)
        self.res, self.ev = self.rx.alloc_result(), self.rx.alloc_events()
        self.sub = self.tx.alloc_submit_result(self.ev.max_events)
        self.busy = torch.zeros(P, dtype=torch.int32, device=DEV)
        self.dd = self.rx.deduper(depth=8, window=30.0) if dedup else None
        self.keep = self.dd.alloc_verdict(self.ev.max_events) if dedup else None
        self.rows, self.seed = rows, seed

    def tick(self, chunk, stream=None):
        self.rx.push(chunk, out=self.res, events=self.ev, mute=self.tx.on_air, stream=stream)
        self.rx.busy(out=self.busy, stream=stream)
        if self.dd is not None:
            self.dd.filter(self.ev, out=self.keep, stream=stream)
        self.tx.submit_events(self.ev, keep=self.keep, out=self.sub, stream=stream)
        self.tx.pull(T, out=self.rows, hold=self.busy, persist=255, slot=0, seed=self.seed, stream=stream)

    def snap(self):
        keep = self.keep if self.keep is not None else self.busy
        return tuple(x.cpu().numpy().copy() for x in (self.sub.status, self.sub.start, self.sub.n_samples, keep,
                                                      self.busy, self.tx.pending, self.tx.on_air))

    def restart(self):
        self.tx.reset()
        self.rx.reset()
        self.tx.on_air.zero_()
        if self.dd is not None:
            self.dd.reset()

    def close(self):
        for x in (self.rx, self.tx) + (() if self.dd is None else (self.dd,)):
            x.close()


class World:
    """Three stations whose pulls write their rows of the medium's source matrix in place; one tick is every station's
    push -> busy -> filter -> submit_events -> pull and then the mix that makes the next tick's chunks."""

    def __init__(self, torch, dedup):
        self.src = torch.zeros((3 * P, T), dtype=torch.int16, device=DEV)
        self.heard = torch.zeros((3 * P, T), dtype=torch.int16, device=DEV)
        self.medium = LiveMedium.from_matrix(GAIN, P, device=DEV)
        self.st = [Station(torch, self.src[s * P:(s + 1) * P], 11 + s, dedup) for s in range(3)]

    def tick(self, stream=None):
        for s, x in enumerate(self.st):
            x.tick(self.heard[s * P:(s + 1) * P], stream)
        self.medium.mix(self.src, out=self.heard, stream=stream)

    def originate(self):
        a = self.st[0]
        sub = a.tx.submit(list(range(P)), PAYS)
        if a.dd is not None:
            a.dd.note(list(range(P)), PAYS, sub.start + sub.n_samples)

    def snap(self):
        return [x.snap() for x in self.st] + [(self.src.cpu().numpy().copy(), self.heard.cpu().numpy().copy())]

    def close(self):
        for x in self.st:
            x.close()


def drive(world, tick):
    log = []
    for t in range(TICKS):
        if t == 1:
            world.originate()
        tick()
        log.append(world.snap())
    return log


def episodes(log, s):
    """How often each channel of station s went on air: the rising edges of its on_air range over the ticks."""
    on = np.array([(e[s][6][:, 1] > e[s][6][:, 0]) for e in log])
    return (on[1:] & ~on[:-1]).sum(axis=0) + on[0]


def test_without_the_filter_the_chain_never_goes_quiet(torch_cuda):
    torch = torch_cuda
    world = World(torch, dedup=False)
    log = drive(world, world.tick)
    torch.cuda.synchronize()
    world.close()
    assert any(e[3][0].any() for e in log[-8:])                     # tones in the last ticks before the bound
    assert (episodes(log, 1) >= 3).all() and (episodes(log, 0) >= 3).all()     # B repeats A and C, who repeat B, ...


def test_with_the_filter_every_station_is_on_air_once_and_one_graph_replays_the_tick(torch_cuda):
    torch = torch_cuda
    world = World(torch, dedup=True)
    log = drive(world, world.tick)
    torch.cuda.synchronize()
    world.close()
    for s in range(3):
        assert episodes(log, s).tolist() == [1] * P, s                # A, B and C: on air exactly once per channel
    queued = [sum(int((e[s][0] == Q).sum()) for e in log) for s in range(3)]
    dup = [sum(int((e[s][0] == D.DUPLICATE).sum()) for e in log) for s in range(3)]
    assert queued == [0, P, P] and dup == [P, P, 0]                   # A drops B's echo, B drops C's
    active = [t for t, e in enumerate(log) if e[3][0].any() or e[3][1].any() or any(e[s][5].any() for s in range(3))]
    assert active and active[-1] <= TICKS - 5                       # then silent for at least four ticks
    # the same ticks as ONE captured graph
    world = World(torch, dedup=True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            world.tick(stream=side)
    torch.cuda.synchronize()
    for x in world.st:                                              # (the capture ran nothing; start from a clean state)
        x.restart()
    world.src.zero_()
    world.heard.zero_()
    torch.cuda.synchronize()
    replayed = drive(world, graph.replay)
    for t, (got, want) in enumerate(zip(replayed, log)):
        for s in range(3):
            for g, w, name in zip(got[s], want[s], NAMES):
                assert (g == w).all(), (t, s, name)
        assert (got[3][0] == want[3][0]).all() and (got[3][1] == want[3][1]).all(), t
    torch.cuda.synchronize()
    del graph
    world.close()
