"""GPU parity (-m gpu) of the relay submit (``afsk_live_tx_submit_events``, ``LiveTransmitter.submit_events``).

Expected values never come from the relay kernels.  Hand-made event buffers are packed by the numpy model
(tests/live_events_model.py) and decided by the relay model (tests/live_relay_model.py, which hands the relayable
records to ``LiveTxModel``); the expected samples are ``Transmitter.wav_samples`` where the queue model puts them, and a twin
transmitter is given the same messages through the host ``submit``.  Real receivers are compared with what their own
packed list holds on the host, and the relayed signal is decoded again by a second receiver.  Integer outputs and
samples: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from afskmodem_amd import _native, batch, live
from afskmodem_amd.live import LiveReceiver, LiveTransmitter
from tests import live_events_model as M
from tests import live_relay_model as R
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_tx_model import LiveTxModel
from tests.test_gpu_live_tx import wav_cache
from tests.test_live_relay_host import hand_buffer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, MARKER = 0x5A, 0xEE
Q, FULL, LONG, BAD, UNSORTED = (_native.LIVE_TX_QUEUED, _native.LIVE_TX_QUEUE_FULL, _native.LIVE_TX_TOO_LONG,
                                _native.LIVE_TX_BAD_CHANNEL, _native.LIVE_TX_UNSORTED)
SKIPPED, NONE = _native.LIVE_TX_SKIPPED, _native.LIVE_TX_NONE
BAUD, BF = 12000, 4          # the hand-made lists' transmitters: short messages, several of a queue inside 8048 samples
WAV = wav_cache(BAUD, 0.0)


def device_events(torch, host_buf, n_rx, slots, stride, max_events, max_bytes):
    """``host_buf`` (the model's events buffer, without the scratch) on the device as a ``LiveEvents`` of a push of
    ``n_rx`` channels, ``slots`` slots and rows of ``stride`` bytes; and the whole buffer as uploaded."""
    ro, po, total = live.events_layout(n_rx, slots, max_events, max_bytes)
    whole = np.full(total, FILL, np.uint8)
    whole[: host_buf.size] = host_buf
    shape = live.LiveResult(np.zeros(n_rx, np.int32), None, np.zeros((n_rx, slots), np.int32), None,
                            batch.HostDemodResult(np.zeros((n_rx * slots, stride), np.uint8), *[None] * 5))
    return live.LiveEvents(torch.from_numpy(whole).to(DEV), max_events, max_bytes, ro, po, result=shape), whole


def assert_outputs(res, want, tag):
    for g, w, name in zip(res.cpu(), want[:3], ("status", "start", "n_samples")):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        assert (g == w).all(), (tag, name, np.nonzero(g != w)[0][:5], g[g != w][:5], w[g != w][:5])


def assert_pulls(torch, tx, model, twin, tag, sizes=(2048, 6000)):
    for T in sizes:
        got = tx.pull(T)
        exp = model.expected(T)
        pend = model.pull(T)
        bad = np.nonzero((got.cpu().numpy() != exp).any(axis=1))[0]
        assert bad.size == 0, (tag, T, bad[:5])
        assert (tx.pending.cpu().numpy() == pend).all(), (tag, T)
        if twin is not None:
            assert torch.equal(got, twin.pull(T)), (tag, T)
            assert torch.equal(tx.pending, twin.pending), (tag, T)


# ------------------------------------------------------------------------------------------------- hand-made lists

def hand_cases(n_rx):
    """The cases of one receiver size, the same on every call: every slots x out_stride x pattern, and over them the
    maps, queue depths, payload capacities below and above out_stride, skip_flags and a transmitter that is idle or
    already holds and has retired messages, each drawn from the case's own seed."""
    out = []
    for slots in (1, 2, 3):
        for stride in (12, 172):
            for pattern in ("zero", "sparse", "full"):
                k = len(out)
                rng = np.random.default_rng(7000 + 100 * n_rx + k)
                arrays = M.random_push(rng, n_rx, slots, stride, pattern, MARKER)
                used = arrays[5]["status"] != 0x7fffffff
                # most bursts decoded: status ST_OK (random_push draws it from -50 ... 2^20)
                arrays[5]["status"][used & (rng.random(n_rx * slots) < 0.85)] = _native.ST_OK
                kind = ("identity", "permutation", "drops")[(k + k // 3) % 3]
                n_tx = n_rx if kind == "identity" else n_rx + 5
                cmap = None
                if kind != "identity":
                    cmap = rng.permutation(n_tx)[:n_rx].astype(np.int32)
                if kind == "drops":
                    draw = rng.random(n_rx)
                    cmap[draw < 0.25] = -rng.integers(1, 9, int((draw < 0.25).sum()))
                    cmap[draw > 0.75] = n_tx + rng.integers(0, 9, int((draw > 0.75).sum()))
                    if n_rx == 1:
                        cmap[0] = (-1, n_tx, 0)[k % 3]
                out.append(dict(n_rx=n_rx, slots=slots, stride=stride, pattern=pattern, arrays=arrays, kind=kind,
                                n_tx=n_tx, cmap=cmap, depth=(1, 2, 4)[(k // 2 + k // 6) % 3],
                                max_payload=stride + (4 if (k + k // 9) % 2 else -4),
                                skip=(_native.LIVE_OPEN_END, 0, 3)[(k // 4) % 3], preload=k % 2 == 1, tag=(n_rx, k)))
    return out


def preload(case):
    """Messages queued ahead of the relay: one byte on every third transmitter channel, retired by a pull of 5000
    samples, so that those channels' rings start at entry 1 and their streams at 5000."""
    chans = list(range(0, case["n_tx"], 3))
    return chans, [bytes([65 + c % 26]) for c in chans]


def model_of(case):
    model = LiveTxModel(case["n_tx"], BF, 0, case["depth"], case["max_payload"], wav=WAV)
    if case["preload"]:
        assert (model.submit(*preload(case))[0] == Q).all()
        assert not model.pull(5000).any()
    return model


def model_relay(case, model):
    n_rx, slots, stride = case["n_rx"], case["slots"], case["stride"]
    me, mb = n_rx * slots, n_rx * slots * stride
    h, recs, pay = M.pack(*case["arrays"], me, mb)
    buf = M.buffer(h, recs, pay, me, mb, FILL)
    return buf, me, mb, R.relay(model, buf, me, mb, stride, n_rx, case["cmap"], case["skip"])


@pytest.mark.parametrize("n_rx", [1, 64, 65, 300])
def test_hand_made_lists_queue_as_the_model_queues_them(torch_cuda, n_rx):
    torch = torch_cuda
    for case in hand_cases(n_rx):
        model = model_of(case)
        buf, me, mb, want = model_relay(case, model)
        ev, whole = device_events(torch, buf, n_rx, case["slots"], case["stride"], me, mb)
        tx, twin = (LiveTransmitter(case["n_tx"], BAUD, 0.0, queue_depth=case["depth"],
                                    max_payload_len=case["max_payload"], device=DEV) for _ in range(2))
        if case["preload"]:
            for t in (tx, twin):
                t.submit(*preload(case))
                t.pull(5000)
        res = tx.submit_events(ev, channel_map=None if case["cmap"] is None else case["cmap"].tolist(),
                               skip_flags=case["skip"])
        assert_outputs(res, want, case["tag"])
        assert (ev.buffer.cpu().numpy() == whole).all(), case["tag"]          # nothing of the events buffer is written
        queued = want[3]
        twin.submit([d for d, _ in queued], [p for _, p in queued])
        assert_pulls(torch, tx, model, twin, case["tag"])
        torch.cuda.synchronize()
        tx.close()
        twin.close()


def test_the_hand_made_cases_reach_every_status_and_every_parameter():
    """What the parametrised test above compares entry by entry with the model, seen from the model alone: no status,
    map kind, queue depth or capacity is left out silently."""
    seen, kinds, depths, caps, skips, relayed_open_end = set(), set(), set(), set(), set(), 0
    for n_rx in (1, 64, 65, 300):
        cases = hand_cases(n_rx)
        assert len(cases) == 18
        for case in cases:
            buf, me, mb, (status, start, ns, queued) = model_relay(case, model_of(case))
            seen |= set(status.tolist())
            kinds.add(case["kind"])
            depths.add(case["depth"])
            caps.add(case["max_payload"] - case["stride"])
            skips.add(case["skip"])
            _, recs, _ = R.parts(buf, me, mb)
            relayed_open_end += int(((recs["flags"][: status.size] & 1) != 0)[status == Q].sum())
            if case["pattern"] == "zero":
                assert (status == NONE).all()
    assert seen == {Q, FULL, LONG, BAD, SKIPPED, NONE}          # (UNSORTED: test_an_unsorted_list_... below)
    assert kinds == {"identity", "permutation", "drops"} and depths == {1, 2, 4} and caps == {-4, 4}
    assert skips == {0, 1, 3} and relayed_open_end > 0


def test_an_unsorted_list_is_refused_from_its_first_descending_record_on(torch_cuda):
    torch = torch_cuda
    rows = [(0, 0, 0, 3, 0), (2, 0, 0, 3, 3), (2, 0, 0, 2, 6), (4, 0, 0, 1, 8), (5, 0, 0, 1, 9), (6, 0, 0, 1, 10),
            (6, 2, 0, 1, 11)]
    for n_sorted in (len(rows), 4, 1):                     # sorted; a channel below its predecessor's at 4; at 1
        use = rows if n_sorted == len(rows) else rows[:n_sorted] + [(-1, 0, 0, 1, 12)] + rows[n_sorted:]
        buf = hand_buffer(use, 9, 16)
        model = LiveTxModel(8, BF, 0, 2, 8, wav=WAV)
        want = R.relay(model, buf, 9, 16, 8, 8)
        status = want[0].tolist()
        if n_sorted == len(rows):
            assert UNSORTED not in status and status[-3:] == [SKIPPED, NONE, NONE]
        else:
            assert status[n_sorted:] == [UNSORTED] * (len(use) - n_sorted) + [NONE]
            assert UNSORTED not in status[:n_sorted]
        ev, whole = device_events(torch, buf, 8, 2, 8, 9, 16)
        tx = LiveTransmitter(8, BAUD, 0.0, queue_depth=2, max_payload_len=8, device=DEV)
        assert_outputs(tx.submit_events(ev), want, n_sorted)
        assert_pulls(torch, tx, model, None, n_sorted)
        assert (ev.buffer.cpu().numpy() == whole).all()
        torch.cuda.synchronize()
        tx.close()


def test_a_long_list_is_refused_from_a_descending_record_anywhere_in_it(torch_cuda):
    """9000 records, one of them given a channel below its predecessor's: at the list's second record, around the
    1024 pairs the order kernel's threads look at side by side, around the 8192 pairs they take per step, at the end."""
    torch = torch_cuda
    n, slots, stride = 3000, 3, 12
    rng = np.random.default_rng(31)
    arrays = M.random_push(rng, n, slots, stride, "full", MARKER)
    arrays[5]["status"][:] = _native.ST_OK
    me, mb = n * slots, n * slots * stride
    h, recs, pay = M.pack(*arrays, me, mb)
    tx = LiveTransmitter(n, BAUD, 0.0, queue_depth=2, max_payload_len=16, device=DEV)
    model = LiveTxModel(n, BF, 0, 2, 16, wav=WAV)
    for k in (1, 1023, 1024, 1025, 8191, 8192, 8193, 8999, None):
        bad = recs.copy()
        if k is not None:
            bad["channel"][k] = bad["channel"][k - 1] - 1
        buf = M.buffer(h, bad, pay, me, mb, FILL)
        tx.reset()
        model.reset()
        want = R.relay(model, buf, me, mb, stride, n)
        status = want[0]
        if k is None:
            assert UNSORTED not in status and NONE not in status
        else:
            assert (status[k:] == UNSORTED).all() and UNSORTED not in status[:k]
        ev, whole = device_events(torch, buf, n, slots, stride, me, mb)
        assert_outputs(tx.submit_events(ev), want, k)
        assert (ev.buffer.cpu().numpy() == whole).all(), k
        assert_pulls(torch, tx, model, None, k, sizes=(1500,))
    torch.cuda.synchronize()
    tx.close()


# ----------------------------------------------------------------------------------------------- the payload copy

SIZES = (1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 1000)


def copy_list(seed, order):
    """16 groups of records of every size in SIZES back to back, group g behind a pad that puts it at residue g mod 16
    and belongs to a record that is not relayed (status NO_DATA): the source offsets of every size take every residue
    mod 16.  Record i is channel i's.  Returns (rows, payload part)."""
    rng = np.random.default_rng(seed)
    rows, off = [], 0
    for g in range(16):
        pad = (g - off) % 16                               # the group's first payload starts at residue g
        rows.append((len(rows), 0, _native.ST_NO_DATA, max(pad, 1), off))
        off += pad
        for nb in order:
            rows.append((len(rows), 0, 0, nb, off))
            off += nb
    return rows, bytes(rng.integers(0, 256, off, dtype=np.uint8))


@pytest.mark.parametrize("max_payload", [1000, 1001, 1003])
def test_payloads_of_every_size_and_alignment_are_copied_exactly(torch_cuda, max_payload):
    torch = torch_cuda
    first, second = copy_list(1, SIZES), copy_list(2, SIZES[::-1])
    n = len(first[0])
    assert n == 16 * 13
    for nb in SIZES:
        assert {off % 16 for _, _, st, k, off in first[0] if st == 0 and k == nb} == set(range(16))
    tx = LiveTransmitter(n, BAUD, 0.0, queue_depth=2, max_payload_len=max_payload, device=DEV)
    model = LiveTxModel(n, BF, 0, 2, max_payload, wav=WAV)
    for rows, pay in (first, second):                 # the second list goes into the next ring entry of every channel
        mb = len(pay)
        buf = hand_buffer(rows, n, mb, payload=pay)
        want = R.relay(model, buf, n, mb, 1000, n)
        assert sorted(set(want[0].tolist())) == [Q, SKIPPED] and (want[0] == SKIPPED).sum() == 16
        ev, whole = device_events(torch, buf, n, 1, 1000, n, mb)
        assert_outputs(tx.submit_events(ev), want, max_payload)
        assert (ev.buffer.cpu().numpy() == whole).all()
    longest = 2 * (BF * (4 + 14 * 1000) + 4800)
    assert_pulls(torch, tx, model, None, max_payload, sizes=(longest // 2 + 77, longest // 2))
    assert not model.pending().any()
    torch.cuda.synchronize()
    tx.close()


# ---------------------------------------------------------------------------------------- capacity-limited lists

def test_lists_one_record_and_one_byte_too_small(torch_cuda):
    """The capacities of test_gpu_live_events.py::test_capacities_bound_what_is_written: records past ``stored`` get
    NONE, records whose payload the pack left out (payload_offset -1) get SKIPPED."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    n, slots, stride = 2 * 256 + 150, 2, 172
    arrays = M.random_push(rng, n, slots, stride, "sparse", MARKER)
    arrays[5]["status"][arrays[5]["status"] != 0x7fffffff] = _native.ST_OK
    arrays[3][arrays[3] != 0x7fff] = 0                                       # no flags: only the capacities skip
    full, all_recs, _ = M.pack(*arrays, n * slots, n * slots * stride)
    count, kept = int(full["count"][0]), int(full["n_bytes"][0])
    assert count > 8 and kept > 400
    for max_events in (count - 1, count, count + 1):
        for max_bytes in (kept - 1, kept, kept + 1):
            h, recs, pay = M.pack(*arrays, max_events, max_bytes)
            buf = M.buffer(h, recs, pay, max_events, max_bytes, FILL)
            model = LiveTxModel(n, BF, 0, 2, 256, wav=WAV)
            want = R.relay(model, buf, max_events, max_bytes, stride, n)
            stored = min(count, max_events)
            assert (want[0][stored:] == NONE).all() and (want[0][:stored] != NONE).all()
            cut = recs["payload_offset"] == -1
            assert cut.any() if max_bytes < kept and max_events >= count else not cut.any() or max_bytes < kept
            assert (want[0][:stored][cut] == SKIPPED).all()
            relayable = (recs["nbytes"] >= 1) & (recs["nbytes"] <= stride) & ~cut
            assert (want[0][:stored][relayable] == Q).all() and relayable.sum() > 4
            ev, whole = device_events(torch, buf, n, slots, stride, max_events, max_bytes)
            tx = LiveTransmitter(n, BAUD, 0.0, queue_depth=2, max_payload_len=256, device=DEV)
            assert_outputs(tx.submit_events(ev), want, (max_events, max_bytes))
            assert (ev.buffer.cpu().numpy() == whole).all()
            assert_pulls(torch, tx, model, None, (max_events, max_bytes))
            torch.cuda.synchronize()
            tx.close()


# ------------------------------------------------------------------------------------------------- real receivers

CHUNK = 8192


def relay_station(torch, kind, rx_bf, lens, n=70, training=0.1, flush_at=None, skip=None, max_payload_len=256,
                  max_burst_len=96000):
    """A source transmitter plays two messages per channel (payload lengths drawn from ``lens``) into receiver A
    (``kind``: "stored" / "stream"), whose packed list of every push is relayed through a permutation map onto
    transmitter B, whose pull is pushed into receiver B (a stored receiver at the relay's rates), tick by tick of CHUNK
    samples.  ``rx_bf``: one bit_frames or one per channel of A; B's channel ``cmap[c]`` runs at channel c's.  A source
    message is queued at the start of a tick (not the first) on an idle channel, as in
    test_gpu_live_rates.py::test_rx_loopback_all_rates, and so is every relayed one.  ``flush_at``: the tick at whose
    end receiver A is flushed.  Returns (per destination channel the payloads the host finds relayable in A's lists,
    what receiver B reports per channel, the records of every tick with their statuses, the payloads, the map)."""
    rng = np.random.default_rng(len(lens) * 1000 + n)
    mixed = np.ndim(rx_bf) > 0
    src = LiveTransmitter(n, [48000 // bf for bf in rx_bf] if mixed else 48000 // rx_bf, training, queue_depth=2,
                          max_payload_len=64, device=DEV)
    pays = [bytes(rng.integers(0, 256, int(rng.choice(lens)), dtype=np.uint8)) for _ in range(2 * n)]
    left = [pays[2 * c: 2 * c + 2] for c in range(n)]
    stream = kind == "stream"
    rx_a = LiveReceiver(n, rx_bf, max_burst_len=None if stream else max_burst_len, max_chunk_len=CHUNK, device=DEV,
                        **(dict(max_payload_len=max_payload_len) if stream else {}))
    n_tx = n + 5
    cmap = np.random.default_rng(5).permutation(n_tx)[:n].astype(np.int32)
    rates = np.full(n_tx, rx_bf[0] if mixed else rx_bf, np.int64)
    if mixed:
        rates[cmap] = np.asarray(rx_bf)
    tx_b = LiveTransmitter(n_tx, (48000 // rates).tolist(), training, queue_depth=8, max_payload_len=64, device=DEV)
    rx_b = LiveReceiver(n_tx, rates.tolist(), max_burst_len=96000, max_chunk_len=CHUNK, device=DEV)
    ev = rx_a.alloc_events()
    out = tx_b.alloc_submit_result(ev.max_events)
    # the statuses of a queue that never fills need no geometry (B's queues are deep enough: checked below)
    model = LiveTxModel(n_tx, 40, 0, 10 ** 9, 64)
    want = [[] for _ in range(n_tx)]
    got = [[] for _ in range(n_tx)]
    log = []
    skip_flags = _native.LIVE_OPEN_END if skip is None else skip
    kw = {} if skip is None else dict(skip_flags=skip)
    busy_until = np.zeros(n, np.int64)
    drained = None                                         # the tick from which on B holds nothing
    for t in range(400):
        pos = t * CHUNK
        idle = [c for c in range(n) if left[c] and busy_until[c] + 2 * 2048 <= pos]
        if idle and t > 0:
            st, s, ns = src.submit(idle, [left[c].pop(0) for c in idle]).cpu()
            assert (st == Q).all() and (s == pos).all()
            busy_until[idle] = s + ns
        sent = not any(left) and busy_until.max() + 3 * CHUNK <= pos
        last = drained is not None and t >= drained + 2
        res = rx_a.push(src.pull(CHUNK), events=ev, flush=t == flush_at)
        tx_b.submit_events(ev, channel_map=cmap.tolist(), out=out, **kw)
        back = rx_b.push(tx_b.pull(CHUNK), flush=last)
        host = ev.buffer.cpu().numpy()
        st, _, _, queued = R.relay(model, host, ev.max_events, ev.max_bytes, rx_a.out_stride, n, cmap, skip_flags)
        got_st = out.status.cpu().numpy()
        assert (got_st == st).all(), (t, got_st[got_st != st][:5], st[got_st != st][:5])
        assert set(st.tolist()) <= {Q, SKIPPED, NONE}, (t, sorted(set(st.tolist())))
        for d, p in queued:
            want[d].append(p)
        assert ev.bursts() == res.bursts(), t
        log.append((ev.records().copy(), st[: ev.stored].copy()))
        for c, _, _, data in back.bursts():
            got[c].append(data)
        if last:
            break
        if sent and drained is None and (tx_b.pending == 0).all().item():
            drained = t
    assert last and (tx_b.pending == 0).all().item() and (src.pending == 0).all().item()
    torch.cuda.synchronize()
    for x in (src, rx_a, tx_b, rx_b):
        x.close()
    return want, got, log, pays, cmap


def all_records(log):
    recs = np.concatenate([r for r, _ in log])
    return recs, np.concatenate([s for _, s in log])


@pytest.mark.parametrize("kind", ["stored", "stream"])
def test_a_relay_repeats_every_payload_on_its_mapped_channel(torch_cuda, kind):
    want, got, log, pays, cmap = relay_station(torch_cuda, kind, 40, lens=(1, 5, 12, 24))
    assert got == want
    for c in range(70):                                    # clean signal, roomy capacities: every payload arrives
        assert got[cmap[c]] == pays[2 * c: 2 * c + 2], c
    recs, st = all_records(log)
    assert (st == Q).all() and recs.size == 140
    assert min(r.size for r, _ in log) == 0 and max(r.size for r, _ in log) > 1


def test_a_mixed_rate_relay_repeats_what_the_receiver_decoded(torch_cuda):
    """bit_frames 4 / 20 / 160 on both ends.  At 12000 baud the reference's .wav quirk destroys the mark tone and no
    payload survives it (test_gpu_live_rates.py): those channels relay what receiver A makes of them, nothing more."""
    rates = [(4, 20, 160)[c % 3] for c in range(70)]
    want, got, log, pays, cmap = relay_station(torch_cuda, "stream", rates, lens=(2, 4, 6), training=0.25)
    assert got == want
    for c in range(70):
        if rates[c] != 4:
            assert got[cmap[c]] == pays[2 * c: 2 * c + 2], (c, rates[c])
    recs, st = all_records(log)
    slow = np.asarray(rates)[recs["channel"]] != 4
    assert (st[slow] == Q).all() and slow.sum() == 2 * sum(r != 4 for r in rates)


def test_truncated_streaming_rows_are_not_relayed(torch_cuda):
    want, got, log, pays, cmap = relay_station(torch_cuda, "stream", 40, lens=(3, 8, 9, 20), max_payload_len=8)
    assert got == want
    recs, st = all_records(log)
    long = recs["nbytes"] > 8
    assert long.any() and (st[long] == SKIPPED).all() and (st[~long] == Q).all() and (~long).any()
    for c in range(70):
        assert got[cmap[c]] == [p for p in pays[2 * c: 2 * c + 2] if len(p) <= 8], c


def test_overflowed_bursts_are_not_relayed(torch_cuda):
    want, got, log, pays, cmap = relay_station(torch_cuda, "stored", 40, lens=(2, 3, 40, 48), max_burst_len=16384)
    assert got == want
    recs, st = all_records(log)
    over = (recs["flags"] & _native.LIVE_OVERFLOW) != 0
    assert over.any() and (st[over] == SKIPPED).all() and (st[~over] == Q).all() and (~over).any()
    for c in range(70):
        assert got[cmap[c]] == [p for p in pays[2 * c: 2 * c + 2] if len(p) <= 3], c


@pytest.mark.parametrize("skip", [None, 0])
def test_bursts_a_flush_reports_open_are_skipped_unless_asked_for(torch_cuda, skip):
    # a message of 5 bytes has 40 * (2 * 60 + 4 + 14 * 5) = 7760 tone samples: queued at the start of tick 1, its tones
    # fill 1616 of the 2048 samples of that tick's last block -- a block amplitude of 0.79 full scale, far above the
    # gate's closing threshold -- so the flush at the end of the tick meets the burst while the gate is still open,
    # the terminator recorded
    tones = 40 * (2 * 60 + 4 + 14 * 5)
    assert 1536 < tones - (CHUNK - 2048) < 2048
    want, got, log, pays, cmap = relay_station(torch_cuda, "stored", 40, lens=(5,), flush_at=1, skip=skip)
    assert got == want
    recs, st = all_records(log)
    open_end = (recs["flags"] & _native.LIVE_OPEN_END) != 0
    assert open_end.any() and not open_end.all()
    if skip is None:
        assert (st[open_end] == SKIPPED).all() and (st[~open_end] == Q).all()
    else:
        ok = recs["status"] == _native.ST_OK
        assert (st[open_end & ok & (recs["nbytes"] > 0)] == Q).all() and (st[~open_end] == Q).all()
        assert (open_end & ok & (recs["nbytes"] > 0)).any()


# ---------------------------------------------------------------------------------------------------------- graph

GT = 4096


@functools.lru_cache(maxsize=None)
def graph_source():
    """[8, 6 * GT] samples: channel c plays one short message from tick c % 3 + 1 on (channels 6 and 7 stay silent), so
    bursts close in some ticks and in others none does."""
    import torch
    src = LiveTransmitter(8, 1200, 0.1, device=DEV)
    chunks = []
    for t in range(6):
        chans = [c for c in range(6) if c % 3 + 1 == t]
        if chans:
            src.submit(chans, [bytes([48 + c, 97 + t, 33]) for c in chans])
        chunks.append(src.pull(GT).cpu().numpy())
    torch.cuda.synchronize()
    src.close()
    return np.concatenate(chunks, axis=1)


def test_a_captured_relay_tick_replays_like_the_eager_calls(torch_cuda):
    torch = torch_cuda
    host = graph_source()
    dev = torch.from_numpy(host).to(DEV)
    cmap = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], dtype=torch.int32, device=DEV)

    def station():
        rx = LiveReceiver(8, 40, max_burst_len=16384, max_chunk_len=GT, device=DEV)
        tx = LiveTransmitter(8, 2400, 0.0, queue_depth=2, max_payload_len=8, device=DEV)
        return rx, tx, rx.alloc_result(), rx.alloc_events(), tx.alloc_submit_result(8 * rx.slots)

    rx, tx, res, ev, sub = station()
    eager = []
    for t in range(6):
        rx.push(dev[:, t * GT:(t + 1) * GT], out=res, events=ev)
        tx.submit_events(ev, channel_map=cmap, out=sub)
        pulled = tx.pull(GT)
        eager.append(tuple(x.cpu().numpy().copy() for x in (sub.status, sub.start, sub.n_samples, pulled, tx.pending)))
    torch.cuda.synchronize()
    rx.close()
    tx.close()
    queued = [int((e[0] == Q).sum()) for e in eager]
    assert sum(queued) == 6 and 0 in queued and any((e[0] == NONE).all() for e in eager)
    assert all(set(e[0].tolist()) <= {Q, NONE} for e in eager) and any(e[3].any() for e in eager)

    rx, tx, res, ev, sub = station()
    chunk = torch.zeros((8, GT), dtype=torch.int16, device=DEV)
    pulled = torch.zeros((8, GT), dtype=torch.int16, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):             # one linear chain: push, pack, submit, pull
            rx.push(chunk, out=res, events=ev, stream=side)
            tx.submit_events(ev, channel_map=cmap, out=sub, stream=side)
            tx.pull(GT, out=pulled, stream=side)
    torch.cuda.synchronize()
    for t in range(6):
        chunk.copy_(dev[:, t * GT:(t + 1) * GT])
        before = tx.pending.cpu().numpy().copy()
        graph.replay()
        got = tuple(x.cpu().numpy() for x in (sub.status, sub.start, sub.n_samples, pulled, tx.pending))
        for g, w, name in zip(got, eager[t], ("status", "start", "n_samples", "samples", "pending")):
            assert (g == w).all(), (t, name)
        if (got[0] == NONE).all():                             # no burst closed: nothing was queued
            assert (got[1] == -1).all() and (got[2] == 0).all() and (got[4] <= before).all()
    torch.cuda.synchronize()
    del graph
    rx.close()
    tx.close()


# --------------------------------------------------------------------------------------------- argument refusals

def test_refused_arguments_leave_the_transmitter_untouched(torch_cuda):
    torch = torch_cuda
    rows = [(0, 0, 0, 3, 0), (1, 0, 0, 3, 3)]
    buf = hand_buffer(rows, 4, 16)
    ev, whole = device_events(torch, buf, 4, 1, 8, 4, 16)
    tx = LiveTransmitter(4, BAUD, 0.0, queue_depth=2, max_payload_len=8, device=DEV)
    model = LiveTxModel(4, BF, 0, 2, 8, wav=WAV)
    tx.submit([2], [b"xy"])
    model.submit([2], [b"xy"])
    sentinel = lambda dt: torch.full((4,), 77, dtype=dt, device=DEV)  # noqa: E731
    st, start, ns = sentinel(torch.int32), sentinel(torch.int64), sentinel(torch.int32)
    p = ev.buffer.data_ptr()
    good = dict(tx=tx.handle, events=p, max_events=4, max_bytes=16, out_stride=8, n_rx=4, map=None, skip=1,
                st=st.data_ptr(), start=start.data_ptr(), ns=ns.data_ptr(), stream=None)
    refusals = [("tx", None), ("events", None), ("st", None), ("start", None), ("ns", None), ("max_events", -1),
                ("max_bytes", -1), ("out_stride", -1), ("n_rx", 0), ("n_rx", -1), ("skip", 4), ("skip", 7),
                ("events", p + 8), ("events", p + 4)]
    for key, value in refusals:
        rc = _native.lib().afsk_live_tx_submit_events(*dict(good, **{key: value}).values())
        assert rc == _native.E_INVALID_ARG, (key, value)
    assert _native.lib().afsk_live_tx_submit_events(*dict(good, max_events=0).values()) == 0
    torch.cuda.synchronize()
    assert all((t == 77).all().item() for t in (st, start, ns))              # nothing was launched
    assert (ev.buffer.cpu().numpy() == whole).all()
    # the Python layer's own refusals
    with pytest.raises(TypeError):
        tx.submit_events(ev.buffer)
    with pytest.raises(ValueError):
        tx.submit_events(live.LiveEvents(whole, 4, 16, result=ev.result))    # a host buffer
    with pytest.raises(ValueError):
        tx.submit_events(live.LiveEvents(ev.buffer, 4, 16))                  # no result: no receiver sizes
    with pytest.raises(ValueError):
        tx.submit_events(ev, skip_flags=4)
    with pytest.raises(ValueError):
        tx.submit_events(ev, channel_map=[0, 1, 2])                          # not one entry per receiver channel
    with pytest.raises(_native.AfskNativeError) as ei:
        tx.submit_events(ev, channel_map=[0, 1, 1, 3])
    assert ei.value.code == _native.E_INVALID_ARG and "1 and 2" in str(ei.value)
    with pytest.raises(TypeError):
        tx.submit_events(ev, channel_map=torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        tx.submit_events(ev, out=tx.alloc_submit_result(5))
    assert_pulls(torch, tx, model, None, "untouched", sizes=(3000, 3000))
    # and the accepted call goes through: the same host map twice is uploaded once
    want = R.relay(model, buf, 4, 16, 8, 4, [3, -1, 0, 1])
    res = tx.submit_events(ev, channel_map=[3, -1, 0, 1])
    first = tx._relay_map_cache[1]
    assert_outputs(res, want, "accepted")
    assert want[0].tolist() == [Q, SKIPPED, NONE, NONE]
    tx.submit_events(ev, channel_map=np.array([3, -1, 0, 1]), out=res)
    assert tx._relay_map_cache[1] is first
    R.relay(model, buf, 4, 16, 8, 4, [3, -1, 0, 1])
    assert_pulls(torch, tx, model, None, "accepted", sizes=(9000,))
    torch.cuda.synchronize()
    tx.close()
