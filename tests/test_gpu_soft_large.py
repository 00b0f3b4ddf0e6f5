"""GPU parity (-m gpu) -- the SOFT outputs (corrected, margins) of the large-launch kernel forms, and where every
form writes.  From 4096 streams on (mixed: 6144, bit_frames 4: 8192, bit_frames 8: 16384; L2 warming: 8192) the
one-wave kernels run another instantiation of their round loops: tail hint armed, partial rounds that may run twice,
the ODD forms -- and each round loop's margin stores sit inside exactly that code.  Every launch here writes into
buffers whose surroundings hold sentinels (tests/soft_cases.py): bytes past nbytes, margins past the symbols the
stream has, rows of refused streams and the neighbours of every array must come back untouched, and every value
must equal the CPU oracle's row of the stream's prototype.  Integer path: tolerance zero.

The stream counts are tied to afsk_demod_ring.h by tests/test_soft_cases_host.py."""
import numpy as np
import pytest

from afskmodem_amd import _native, batch, live
from oracle import afsk_oracle as O
from tests import soft_cases as S
from tests.gpu_common import REAL_DEMOD_BATCH, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def upload(torch, launch):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return t(launch.flat), t(launch.off), t(launch.lens)


def run_entry(torch, launch, entry, out_stride=S.OUT_STRIDE, margin_stride=None, dev=None, out=None):
    """One launch of ``launch`` through ``entry`` into guarded outputs (``out``: reuse them), then the footprint check."""
    x, off, ln = dev if dev is not None else upload(torch, launch)
    ln = ln if dev is None else torch.from_numpy(launch.lens).to(DEV)
    n = launch.lens.size
    if out is None:
        out = S.guarded_result(n, out_stride, margin_stride or launch.margin_stride, DEV)
    if entry == "split":
        plan = batch.SplitPlan(launch.host_lens, launch.bf, DEV, segment_symbols=64)
        res = batch.demod_batch_split(x, off, ln, plan, 14000, out=out, diagnostics=True)
    else:
        if entry == "uniform":
            assert (launch.bf == launch.bf[0]).all()
            bf = int(launch.bf[0])
        elif entry == "mixed":
            bf = torch.from_numpy(launch.bf).to(DEV)                     # bit_frames on the device
        else:
            bf = launch.bf                                               # the plan comes from the host's, invalid ones included
        res = REAL_DEMOD_BATCH(x, off, ln, bf, 14000, out=out, validate=False, diagnostics=True, entry=entry)
    assert res is out
    torch.cuda.synchronize()
    S.check_footprint(out, out.guards, launch.want, launch.lens, launch.bf, one_wave=entry != "split",
                      tag=f"{entry}, {n} streams")
    return out, (x, off, ln)


def mixed_set():
    ps = S.merged(S.MIXED_BIT_FRAMES)
    S.assert_conditions(ps, mixed=True)
    return ps


@pytest.mark.parametrize("n", S.N_MIXED)
def test_mixed_entry_large_launch(torch_cuda, n):
    """bit_frames on the device, all 30 rates plus two run-time geometries in one launch: 6200 streams arm the tail
    hint alone, 8256 the hint and the L2 warming.  Refused lengths and bit_frames sit between decoded streams."""
    launch = S.build_launch(mixed_set(), n, 100 + n, invalid_bf=True)
    run_entry(torch_cuda, launch, "mixed")


@pytest.mark.parametrize("n", S.N_GROUPED)
def test_grouped_entry_large_launch(torch_cuda, n):
    """The same rates through the rate-sorted walk (4200: armed for it and not for the per-stream entry); the plan
    comes from the host bit_frames, whose invalid values land in its refused bucket."""
    launch = S.build_launch(mixed_set(), n, 200 + n, invalid_bf=True)
    run_entry(torch_cuda, launch, "grouped")


UNIFORM_GROUPS = [S.ALL_BIT_FRAMES[i: i + 6] for i in range(0, len(S.ALL_BIT_FRAMES), 6)]


@pytest.mark.parametrize("group", UNIFORM_GROUPS, ids=lambda g: "bf" + "_".join(str(b) for b in g))
def test_uniform_entry_large_launch_every_geometry(torch_cuda, group):
    """Every one of the 36 compile-time geometries and both run-time ones in a uniform launch above its own threshold
    (8256 streams: hint and warming; bit_frames 8: 16500), one launch per rate."""
    for bf in group:
        ps = S.prototypes(bf)
        S.assert_conditions(ps)
        n = S.N_UNIFORM_BF8 if bf == 8 else S.N_UNIFORM
        run_entry(torch_cuda, S.build_launch(ps, n, 300 + bf), "uniform")


@pytest.mark.parametrize("bf", S.HINT_ONLY_BIT_FRAMES)
def test_uniform_entry_hint_without_warming(torch_cuda, bf):
    """4200 streams: the large form with the tail hint and without the warming requests in the in-flight count, one
    rate per round-loop family (fast: 40, 20, 160; multi: 16, 48; wm: 100, 320; gp: 128, 1000; run-time: 136)."""
    ps = S.prototypes(bf)
    S.assert_conditions(ps)
    run_entry(torch_cuda, S.build_launch(ps, S.N_HINT_ONLY, 400 + bf), "uniform")


@pytest.mark.parametrize("entry", ["mixed", "uniform"])
def test_narrow_strides_truncate_rows_without_touching_the_neighbours(torch_cuda, entry):
    """out_stride 5 and margin_stride 37: both truncate, both are odd, neither is a multiple of a lane count.
    nbytes (and the symbol count) still report the full figures; refused rows between truncated ones stay untouched."""
    if entry == "mixed":
        launch = S.build_launch(mixed_set(), S.N_MIXED[0], 100 + S.N_MIXED[0], invalid_bf=True)
    else:
        launch = S.build_launch(S.prototypes(40), S.N_HINT_ONLY, 440)
    w = launch.want
    assert (w["nbytes"] > S.NARROW_OUT_STRIDE).any() and (w["n_symbols"] > S.NARROW_MARGIN_STRIDE).sum() > launch.lens.size // 2
    run_entry(torch_cuda, launch, entry, out_stride=S.NARROW_OUT_STRIDE, margin_stride=S.NARROW_MARGIN_STRIDE)


SMALL_BIT_FRAMES = (40, 8, 1000, 136, 100, 16)


@pytest.mark.parametrize("entry", ["mixed", "grouped", "uniform", "split"])
def test_small_launch_forms_and_split_path_footprint(torch_cuda, entry):
    """The prototypes once, without tiling (about 300 streams: the small-launch kernels), and the sequence-parallel
    path with 64-symbol segments: their values are compared elsewhere too, their write footprint only here."""
    torch = torch_cuda
    if entry == "uniform":
        for bf in SMALL_BIT_FRAMES:
            run_entry(torch, S.build_launch(S.prototypes(bf), None, 0), "uniform")
        return
    # (a split plan takes a Receiver's rates only: no run-time geometry, no invalid bit_frames)
    ps = S.merged([b for b in SMALL_BIT_FRAMES if entry != "split" or 48000 % b == 0])
    launch = S.build_launch(ps, None, 0, invalid_bf=entry != "split")
    assert launch.lens.size <= S.N_SMALL_MAX
    run_entry(torch, launch, entry)
    if entry == "split":                       # its rows truncate like the others'
        run_entry(torch, launch, entry, out_stride=S.NARROW_OUT_STRIDE, margin_stride=S.NARROW_MARGIN_STRIDE)


@pytest.mark.parametrize("entry", ["mixed", "grouped", "uniform", "split"])
def test_reused_outputs_report_no_corrections_for_refused_streams(torch_cuda, entry):
    """out= reuse: launch 1 decodes the forced-correction prototypes (corrected > 0); launch 2 goes into the SAME
    result with the device stream_len rewritten so that every second stream is refused (0, 4095, -1).  A refused
    stream reports corrected == 0 -- not the count of whatever used its slot before -- and the whole footprint is
    launch 2's."""
    torch = torch_cuda
    ps = S.prototypes(40)
    P = len(ps.streams)
    order = np.concatenate([ps.forced, ps.forced, np.arange(P)])       # slots 0 ... 5: forced ones at even and odd slots
    sub = S.ProtoSet(tuple(ps.streams[i] for i in order), ps.lens[order], ps.bf[order],
                     {k: v[order] for k, v in ps.want.items()}, np.arange(3))
    first = S.build_launch(sub, None, 0, refused_every=0)
    assert (first.want["corrected"][:6] > 0).all()
    out, dev = run_entry(torch, first, entry)
    got = out.corrected.cpu().numpy()
    assert (got[:6] == first.want["corrected"][:6]).all() and (got[:6] > 0).all()
    second = S.refuse(first, np.arange(1, first.lens.size, 2), S.REFUSED_LENGTHS)
    assert second.refused[[1, 3, 5]].all() and (first.want["corrected"][[1, 3, 5]] > 0).all()
    # the rows get their sentinels back (a refused stream leaves its rows alone, so launch 1's bytes and margins
    # would still stand there); the int32 arrays, corrected among them, keep what launch 1 wrote
    out.guards.bytes.fill_(S.BYTE_SENTINEL)
    out.guards.margins.fill_(S.MARGIN_SENTINEL)
    run_entry(torch, second, entry, dev=dev, out=out)
    assert (out.corrected.cpu().numpy()[1::2] == 0).all()


def test_stored_live_receiver_unused_slots_report_no_corrections(torch_cuda):
    """The stored live receiver reuses one result for every push and hands unused slots to the demodulator as
    length 0.  One push closes a burst made from a forced-correction prototype: its slot reports the oracle's corrected
    count for the gated burst (> 0).  The pushes of silence behind it close nothing: every slot then reports
    corrected 0, status TOO_SHORT and 0 bytes."""
    torch = torch_cuda
    ps = S.prototypes(40)
    x = np.asarray(ps.streams[int(ps.forced[0])][: ps.lens[ps.forced[0]]])
    n_ch, T = 3, 8192
    total = -(-(len(x) + 4096) // T) * T + 3 * T                       # silence behind the bursts: pushes that close nothing
    host = np.zeros((n_ch, total), np.int16)
    host[0, 2048: 2048 + len(x)] = x
    host[2, 4096: 4096 + len(x)] = x
    rx = live.LiveReceiver(n_ch, 40, max_burst_len=32768, max_chunk_len=T, device=DEV)
    res = rx.alloc_result(diagnostics=True)
    d = res.demod
    dev = torch.from_numpy(host).to(DEV)
    closed = np.zeros(n_ch, np.int64)
    idle_after = 0
    for p in range(0, total, T):
        rx.push(dev[:, p: p + T], out=res)
        torch.cuda.synchronize()
        n_closed = res.n_closed.cpu().numpy()
        corr, status, nbytes = (a.cpu().numpy().reshape(n_ch, rx.slots) for a in (d.corrected, d.status, d.nbytes))
        used = np.arange(rx.slots)[None, :] < n_closed[:, None]
        for c in np.nonzero(n_closed)[0]:
            assert n_closed[c] == 1 and c in (0, 2)
            b0, bl = int(res.burst_start[c, 0]), int(res.burst_len[c, 0])
            w = O.demod_batch_soft(host[c], [b0], [bl], [40], 14000, out_stride=S.OUT_STRIDE, margin_stride=bl // 40 + 8)
            assert int(w["corrected"][0]) > 0 and int(w["status"][0]) == 0 and int(w["nbytes"][0]) == 5
            assert (int(corr[c, 0]), int(status[c, 0]), int(nbytes[c, 0])) == (int(w["corrected"][0]), 0, 5), (p, c)
        # an unused slot: no corrections, TOO_SHORT, no bytes -- whatever the slot held after an earlier push
        assert (corr[~used] == 0).all(), (p, corr[:, :2])
        assert (status[~used] == _native.ST_TOO_SHORT).all() and (nbytes[~used] == 0).all(), p
        closed += n_closed
        idle_after += int(closed.sum() == 2 and not n_closed.any())
    assert list(closed) == [1, 0, 1] and idle_after >= 2
    rx.close()
