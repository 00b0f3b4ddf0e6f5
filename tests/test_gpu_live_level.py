"""GPU suite of the level tracker (``LiveReceiver(..., level=)``, afsk_live_level.hip): the device's level rows and the
gate they steer against the numpy model (tests/live_level_model.py) bit for bit over plain, ragged, muted and flushing
pushes and a masked reset; one threshold pair per burst (a leveled receiver against a fixed per-channel receiver built
from the pairs the bursts opened with) for every receiver kind, with the packed lists; tracker + push captured into one
graph; and the feature itself -- a listener behind links of gain 1, 1/4 and 1/8 that returns every payload where the
default listener returns the unity link's alone.  70 channels: not a multiple of the four waves of a block."""
import numpy as np
import pytest

from afskmodem_amd import _native, synth
from afskmodem_amd.live import LevelSpec, LiveMedium, LiveReceiver
from oracle import afsk_oracle as O
from tests import live_level_inputs as I
from tests import live_level_model as M
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import FIELDS, collect

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = I.N


def check_bursts(rx, res, want, bf, tag):
    """One push's bursts per channel against the model's: the gate's outputs, and every demod field and payload byte
    against the CPU oracle on the model's burst samples with the pair the burst opened with."""
    got = [[] for _ in range(N)]
    collect(res, got)
    for c in range(N):
        assert [(g["start"], g["len"], g["flags"]) for g in got[c]] == \
            [(w["start"], w["len"], w["flags"]) for w in want[c]], (tag, c)
        for g, w in zip(got[c], want[c]):
            d = O.demod_batch(w["samples"], [0], [w["len"]], [int(bf[c])], w["amp_end"], out_stride=rx.out_stride)
            assert {f: g[f] for f in FIELDS} == {f: int(d[f][0]) for f in FIELDS}, (tag, c)
            assert g["bytes"] == d["bytes"][0, : min(int(d["nbytes"][0]), rx.out_stride)].tobytes(), (tag, c)


@pytest.mark.parametrize("T", [2048, 3000, 8192])
def test_level_rows_and_gate_match_the_model(torch_cuda, T):
    streams = I.parity_streams()
    bf = np.full(N, 40, np.int32)
    rx = LiveReceiver(N, 40, max_burst_len=None, max_payload_len=32, max_chunk_len=T, device=DEV, level=True)
    assert rx.leveled and rx.level_spec == LevelSpec() and tuple(rx.level_state.shape) == (N, 4)
    at = rx.level_state.data_ptr()
    model = M.Receiver(N)
    assert np.array_equal(rx.level_state.cpu().numpy(), model.state)
    out = rx.alloc_result()
    n_bursts = 0
    for i, step in enumerate(I.push_plan(T, I.PARITY_LEN)):
        if step["reset"] is not None:
            rx.reset(step["reset"])
            model.reset(step["reset"])
            assert np.array_equal(rx.level_state.cpu().numpy(), model.state), ("reset", i)
        chunk = I.chunk_of(streams, step, T)
        flush = False if step["flush"] is None else step["flush"]
        res = rx.push(chunk, out=out, lengths=step["lens"], flush=flush, mute=step["mute"])
        want = model.push(chunk, step["lens"], flush, step["mute"])
        assert np.array_equal(rx.level_state.cpu().numpy(), model.state), ("state", i)
        check_bursts(rx, res, want, bf, ("push", i))
        n_bursts += sum(len(w) for w in want)
    want = model.push(np.zeros((N, 0), np.int16), flush=True)
    check_bursts(rx, rx.flush(out=out), want, bf, "flush")
    assert np.array_equal(rx.level_state.cpu().numpy(), model.state)       # (T = 0: no tracker, the rows stay)
    assert rx.level_state.data_ptr() == at and n_bursts >= N // 2
    rx.close()


def snapshot(res):
    """A push's result on the host: every gate and demod output, the payload rows of the closed slots, and what the
    lists built from it say."""
    d = res.demod
    snap = {k: getattr(res, k).cpu().numpy().copy() for k in ("n_closed", "burst_start", "burst_len", "flags")}
    snap.update({k: getattr(d, k).cpu().numpy().copy() for k in FIELDS + ("corrected",)})
    if res.bit_frames is not None:
        snap.update(bit_frames=res.bit_frames.cpu().numpy().copy(), rate_score=res.rate_score.cpu().numpy().copy())
    snap["bursts"] = res.bursts()
    if res.tap is not None:
        snap["partials"] = res.partials()
    if getattr(res, "events", None) is not None:
        snap["events"] = res.events.bursts()
    if getattr(res, "segments", None) is not None:
        snap["segments"] = res.segments.partials()
    return snap


def same_snapshot(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (tag, k)
        else:
            assert a[k] == b[k], (tag, k)


def build(kind, rates, level, start=18000, end=14000, T=I.PAIR_T):
    kw = dict(max_burst_len=None, max_payload_len=32, max_chunk_len=T, device=DEV, level=level)
    if kind == "auto":
        return LiveReceiver(N, "auto", start, end, candidates=[40, 80], **kw)
    return LiveReceiver(N, rates.tolist(), start, end, progressive=kind == "progressive", **kw)


def run(rx, d, T=I.PAIR_T):
    """Every push of d ([N, L] device) and the flush, with the packed lists the receiver has, as snapshots."""
    out = rx.alloc_result(diagnostics=True)
    ev = rx.alloc_events()
    sg = rx.alloc_segments() if rx.progressive else None
    snaps = []
    for p in range(0, d.shape[1], T):
        snaps.append(snapshot(rx.push(d[:, p: p + T], out=out, events=ev, segments=sg)))
    snaps.append(snapshot(rx.flush(out=out, events=ev, segments=sg)))
    return snaps


@pytest.mark.parametrize("kind", ["fixed", "mixed", "auto", "progressive"])
def test_a_burst_keeps_one_pair_and_equals_the_fixed_receiver_of_that_pair(torch_cuda, kind):
    """One burst per channel behind a noise lead-in (tests/test_live_level_host.py checks with the model that the
    lead-in stays under the pair): every output of the leveled receiver, push by push, is the output of the same
    receiver kind built with the pair each channel held when its burst opened."""
    torch = torch_cuda
    rates = I.pair_rates(kind)
    host, sent = I.pair_streams(rates)
    d = torch.from_numpy(host).to(DEV)
    model = M.Receiver(N)
    pairs = np.tile(np.asarray([18000, 14000], np.int32), (N, 1))
    for p in range(0, I.PAIR_LEN, I.PAIR_T):
        for c, bursts in enumerate(model.push(host[:, p: p + I.PAIR_T])):
            for b in bursts:
                pairs[c] = (b["amp_start"], b["amp_end"])
    leveled = build(kind, rates, True)
    got = run(leveled, d)
    assert np.array_equal(leveled.level_state.cpu().numpy(), model.state)
    fixed = build(kind, rates, None, pairs[:, 0].tolist(), pairs[:, 1].tolist())
    assert not fixed.leveled and fixed.level_state is None
    want = run(fixed, d)
    for i, (g, w) in enumerate(zip(got, want)):
        same_snapshot(g, w, (kind, i))
    heard = {c: p for g in got for c, _, _, p in g["bursts"]}
    assert heard == {c: p for c, p in enumerate(sent) if p is not None}
    assert len({tuple(p) for p in pairs.tolist()}) > 20                  # (the channels' pairs do differ)
    leveled.close()
    fixed.close()


def test_tracker_and_push_replay_from_one_graph(torch_cuda):
    torch = torch_cuda
    T = I.PAIR_T
    rates = I.pair_rates("fixed")
    host, _ = I.pair_streams(rates)
    d = torch.from_numpy(host).to(DEV)
    eager, graphed = build("fixed", rates, True), build("fixed", rates, True)
    src = torch.zeros((N, T), dtype=torch.int16, device=DEV)
    out_e, out_g = eager.alloc_result(diagnostics=True), graphed.alloc_result(diagnostics=True)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graphed.push(src, out=out_g, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    graphed.reset()
    n_bursts = 0
    for p in range(0, I.PAIR_LEN, T):
        src.copy_(d[:, p: p + T])
        g.replay()
        eager.push(d[:, p: p + T], out=out_e)
        same_snapshot(snapshot(out_g), snapshot(out_e), ("graph", p))
        assert torch.equal(graphed.level_state, eager.level_state), p
        n_bursts += int(out_e.n_closed.sum())
    same_snapshot(snapshot(graphed.flush(out=out_g)), snapshot(eager.flush(out=out_e)), "flush")
    assert n_bursts >= N // 2
    torch.cuda.synchronize()
    graphed.close()
    eager.close()


def test_a_listener_behind_weak_links_hears_every_station(torch_cuda):
    """Three stations of four channels through LiveMedium.from_matrix at link gains 1, 1/4 and 1/8 into one listener,
    receiver noise at 30 dB: the leveled listener returns every payload, the default one (18000 / 14000) those of the
    unity link alone.  On the parent ``level=`` does not exist."""
    torch = torch_cuda
    P, T = 4, 4096
    gains = [1.0, 0.25, 0.125]
    msgs = [[I.message(40, b"st%d ch%d hello" % (s, c)) for c in range(P)] for s in range(3)]
    span = max(m.size for row in msgs for m in row)
    slot = 48000 + span                                       # a second of idle between the stations' messages
    total = -(-(48000 + 3 * slot) // T) * T
    src = np.zeros((3 * P, total), np.int16)
    for s in range(3):
        for c in range(P):
            at = 48000 + s * slot + 517 * c
            src[s * P + c, at: at + msgs[s][c].size] = msgs[s][c].astype(np.int16)
    d_src = torch.from_numpy(src).to(DEV)
    medium = LiveMedium.from_matrix([gains], P, device=DEV, noise_scale_q24=synth.snr_to_scale_q24(30.0), seed=4)
    kw = dict(max_burst_len=None, max_payload_len=32, max_chunk_len=T, device=DEV)
    leveled, default = LiveReceiver(P, 40, level=True, **kw), LiveReceiver(P, 40, **kw)
    chunk = torch.zeros((P, T), dtype=torch.int16, device=DEV)
    heard = {True: [[] for _ in range(P)], False: [[] for _ in range(P)]}
    outs = {True: leveled.alloc_result(), False: default.alloc_result()}
    for p in range(0, total, T):
        medium.mix(d_src[:, p: p + T], out=chunk)
        for rx in (leveled, default):
            collect(rx.push(chunk, out=outs[rx.leveled]), heard[rx.leveled])
    for rx in (leveled, default):
        collect(rx.flush(out=outs[rx.leveled]), heard[rx.leveled])
    for c in range(P):
        assert [b["bytes"] for b in heard[True][c]] == [b"st%d ch%d hello" % (s, c) for s in range(3)], c
        assert [b["status"] for b in heard[True][c]] == [_native.ST_OK] * 3
        assert [b["bytes"] for b in heard[False][c]] == [b"st0 ch%d hello" % c], c
    torch.cuda.synchronize()
    leveled.close()
    default.close()
