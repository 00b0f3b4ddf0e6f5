"""GPU parity (-m gpu) -- systematic sweeps of the streaming live receiver's sink (afsk_live_stream.hip:
stream_symbols, the incremental terminator search, squelch stop, Hamming decode and byte pack of LiveStreamSinkT) at
symbol, block and tie boundaries: a gate block's edge at every residue inside a symbol, inside the terminator at every
position, at a squelch stop (symbols exactly on the threshold included, a threshold pair per channel), inside a
codeword at every count of pending coded bits, and symbols whose mark and space sums are within one bit_frames of each
other or equal.

The inputs come from tests/live_sweep_inputs.py; every expected value is the CPU oracle's gate and demod of the row,
never the generator's intent and never another GPU path's.  Each sweep first asserts, from the oracle's outputs, that
the placement it was built for happened (the same conditions tests/test_live_sweep_inputs_host.py proves on the CPU).
The same pushes also go through a stored receiver that holds every burst: a failure there too is a gate or input
surprise, a failure of the streaming receiver alone is the sink's.  A thinned mix also goes through the tapped
receiver, the auto receiver with one candidate and ragged pushes; the near ties and the every-codeword streams also go,
as flat batches, through the uniform, per-stream and split entries.  Integer paths: tolerance zero."""
import numpy as np
import pytest

from afskmodem_amd import batch
from afskmodem_amd.live import LiveReceiver
from tests import live_sweep_inputs as L
from tests import split_sweep_inputs as I
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import BLOCK, collect, drive, push_sizes
from tests.test_gpu_split_sweeps import check, poisoned_result, split_launch, uniform_control, upload
from tests.test_live_ragged_host import schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DRAW = [2047, 2048, 5000]                       # what the seeded chunking draws its push sizes from
DRAW_FAR = DRAW + [8192]                        # (8192: the far rows only)
RAGGED = (0, 2047, 2048, 2049, 4000, 6144)      # a channel's own sample count per ragged push


def compare(got, want, tag, rows=None):
    """Every burst of every channel against the expected rows: start, len, flags, every demod field, corrected, the
    bytes -- every key the expected rows have."""
    assert len(got) == len(want), tag
    for c, (g, w) in enumerate(zip(got, want)):
        c = c if rows is None else int(rows[c])
        assert [b["start"] for b in g] == [b["start"] for b in w], (tag, c)
        for gb, wb in zip(g, w):
            for k, v in wb.items():
                assert gb[k] == v, (tag, c, k, gb[k], v)


def receivers(ls, total, chunk, **kw):
    """The stored receiver that holds every burst whole, and the streaming one: one channel per row."""
    pair = (ls.a_start.tolist(), ls.a_end.tolist())
    stored = LiveReceiver(ls.n, ls.bf.tolist(), *pair, max_burst_len=(total // BLOCK + 2) * BLOCK, max_chunk_len=chunk,
                          device=DEV)
    stream = LiveReceiver(ls.n, ls.bf.tolist(), *pair, max_burst_len=None, max_payload_len=ls.maxp, max_chunk_len=chunk,
                          device=DEV, **kw)
    assert stored.slots == stream.slots
    return stored, stream


def sweep(torch, ls, want, seed, far=False):
    """The rows in pushes of 2048, of 2049 (edges drifting through the blocks) and of one seeded chunking, each through
    the stored and the streaming receiver."""
    d = torch.from_numpy(ls.host).to(DEV)
    total = ls.host.shape[1]
    rng = np.random.default_rng(seed)
    for T in (2048, 2049, "random"):
        sizes = push_sizes(T, total, rng, DRAW_FAR if far else DRAW)
        stored, stream = receivers(ls, total, max(sizes))
        got = drive(stored, d, sizes, corrected=True)
        stored.close()
        compare(got, want, f"STORED receiver (a gate or input surprise), pushes of {T}")
        got = drive(stream, d, sizes, corrected=True)
        stream.close()
        compare(got, want, f"streaming receiver, pushes of {T}")
    return stream


def test_block_edge_at_every_residue_inside_a_symbol(torch_cuda):
    """(A) bit_frames 8, 40, 100 (q = 25), 160 and 2000: (j * 2048 - ci) % bf over the block edges j takes every
    residue (160, 2000: 0, 1, bf - 1 and sixteen more) -- residue 0 is the K rule, a symbol that ends on the last
    recorded sample waits --, in bursts a quiet block closes and bursts still loud at the flush."""
    ls, want = L.load("a")
    L.check_a(ls, want)
    sweep(torch_cuda, ls, want, 6001)


def test_terminator_at_every_position(torch_cuda):
    """(B) bit_frames 40, 8, 100: the terminator's last symbol at every index from 3 into the sixth block: decided
    in one go at the lock, split 1|3, 2|2 and 3|1 by the edge between blocks 1 and 2 and by later ones, ending
    exactly on an edge; and a data-like 1,0,0,0 inside the training."""
    ls, want = L.load("b")
    L.check_b(ls, want)
    sweep(torch_cuda, ls, want, 6002)


@pytest.mark.parametrize("far", [False, True], ids=["near", "around_4096"])
def test_squelch_stop_at_every_position(torch_cuda, far):
    """(C) the first dimmed data symbol at 0 ... 140 (``far``: around symbol 4096) -- silent, one below the channel's
    threshold, exactly on it (which does not stop) --, rows squelched at 14000 and at 9000 in ONE receiver: the
    PER_CHANNEL cell of live_push_kernel."""
    ls, want = L.load("c_far" if far else "c")
    L.check_c(ls, want, far)
    assert set(ls.a_end.tolist()) == set(L.C_AMP_ENDS)
    stream = sweep(torch_cuda, ls, want, 6003 + far, far)
    assert stream.amp_end_threshold is None and stream.bit_frames is None      # a pair and a rate per channel


def test_hamming_and_byte_carry(torch_cuda):
    """(D) a block edge at every count of pending coded bits, with and without a held high nibble, through codewords
    with flipped bits; every 7-bit word as a high and as a low nibble (no, single, double and triple errors)."""
    ls, want = L.load("d")
    L.check_d(ls, want)
    sweep(torch_cuda, ls, want, 6005)


def test_near_tie_decisions(torch_cuda):
    """(E) symbols of high, low and dead-zone samples with mark sum M and space sum S: M < S with equal and with
    different quotients by bit_frames, M == S, M > S by less than bit_frames and by more -- at the smallest rate and
    at one rate per lanes-per-symbol value of stream_symbols (1 ... 32 lanes and the cross-lane reduction)."""
    ls, want = L.load("e")
    L.check_e(ls, want)
    sweep(torch_cuda, ls, want, 6006)


# ------------------------------------------------------------------------- the other receivers over a thinned mix

def tapped(torch, ls, want, d, sizes):
    """progressive=True without payload rows: every output but the bytes as expected, the assembler's payloads the
    oracle's bytes."""
    rx = LiveReceiver(ls.n, ls.bf.tolist(), ls.a_start.tolist(), ls.a_end.tolist(), max_burst_len=None,
                      max_payload_len=0, max_chunk_len=max(sizes), progressive=True, device=DEV)
    asm, done = rx.assembler(), []
    got = drive(rx, d, sizes, corrected=True, each=lambda out: done.extend(asm.feed(out)))
    rx.close()
    compare(got, [[{k: v for k, v in b.items() if k != "bytes"} for b in w] for w in want], "tapped receiver")
    assert asm.pending() == {}
    assert sorted(done) == sorted((c, b["start"], b["len"], b["bytes"]) for c, w in enumerate(want) for b in w)


def auto_one_candidate(torch, ls, want, d, sizes):
    """candidates=[bf] on the rows of one rate: bit for bit the fixed-rate answer."""
    for bf in sorted(set(ls.bf.tolist())):
        rows = np.nonzero(ls.bf == bf)[0]
        rx = LiveReceiver(rows.size, "auto", ls.a_start[rows].tolist(), ls.a_end[rows].tolist(), candidates=[bf],
                          max_burst_len=None, max_payload_len=ls.maxp, max_chunk_len=max(sizes), device=DEV)
        got = drive(rx, d[torch.from_numpy(rows).to(DEV)].contiguous(), sizes, corrected=True)
        rx.close()
        compare(got, [want[c] for c in rows], f"auto receiver, candidates [{bf}]", rows)
        assert all(b["bit_frames"] == bf for g in got for b in g)


def ragged(torch, ls, want, d, seed, T):
    """Every channel takes its own seeded number of samples per push and is flushed on its own."""
    total = ls.host.shape[1]
    sched = schedule(np.random.default_rng(seed), [total] * ls.n, T, tuple(x for x in RAGGED if x <= T) + (T,))
    rx = LiveReceiver(ls.n, ls.bf.tolist(), ls.a_start.tolist(), ls.a_end.tolist(), max_burst_len=None,
                      max_payload_len=ls.maxp, max_chunk_len=T, device=DEV)
    got = [[] for _ in range(ls.n)]
    out = rx.alloc_result(diagnostics=True)
    pos = torch.zeros(ls.n, dtype=torch.int64, device=DEV)
    span = torch.arange(T, device=DEV)[None, :]
    assert any(len(set(lens.tolist())) > 1 for lens, _ in sched)                # channels differ within a push
    for lens, mask in sched:
        buf = torch.gather(d, 1, (pos[:, None] + span).clamp_(max=total - 1))      # row c: its next T samples
        d_lens = torch.from_numpy(lens).to(DEV)
        collect(rx.push(buf, out=out, lengths=d_lens, flush=mask.astype(bool) if mask.any() else False), got, True)
        pos += d_lens
    assert (pos == total).all()
    rx.close()
    compare(got, want, "ragged pushes")


@pytest.mark.parametrize("far", [False, True], ids=["near", "around_4096"])
def test_thinned_mix_through_tapped_auto_and_ragged(torch_cuda, far):
    """Every seventh row of (B), (C) and (D) and every row whose placement is an edge case, the rates interleaved."""
    torch = torch_cuda
    ls, want = L.load("mix_far" if far else "mix")
    L.geometry(ls, want)
    assert len(set(ls.bf.tolist())) == 3 and len(set(ls.a_end.tolist())) == 2
    d = torch.from_numpy(ls.host).to(DEV)
    rng = np.random.default_rng(6010 + far)
    sizes = push_sizes("random", ls.host.shape[1], rng, DRAW_FAR if far else DRAW)
    tapped(torch, ls, want, d, sizes)
    auto_one_candidate(torch, ls, want, d, sizes)
    ragged(torch, ls, want, d, 6020 + far, 8192 if far else 6144)


# ---------------------------------------------------------------------------- the batch entries and the split path

def test_near_ties_and_every_codeword_through_the_batch_and_split_entries(torch_cuda):
    """The bursts of (E) and the every-word streams of (D) as one flat batch through the split path (segments of 64 and
    of 1024 symbols, margins included), the uniform entry (one launch per rate) and the per-stream entry: the near
    ties of the other two implementations of the symbol loop.  Outputs poisoned."""
    torch = torch_cuda
    e, want_e = L.load("e")
    d, want_d = L.load("d")
    L.check_e(e, want_e)
    L.check_d(d, want_d)
    every = np.nonzero(d.col("every_word") == 1)[0]
    sw = I.concat(L.as_sweep(e, want_e, range(e.n)), L.as_sweep(d, want_d, every))
    full = int((sw.ln // sw.bf).max()) + 8
    want = I.oracle(sw, soft=full)
    live = [w[0] for w in want_e] + [want_d[c][0] for c in every]
    for f in L.FIELDS + ("corrected",):                        # the same samples: the same answers
        assert want[f].tolist() == [b[f] for b in live], f
    K = I.geometry(sw, want)[2]
    assert (K < full).all() and set(sw.bf.tolist()) == set(L.E_RATES)
    dev = upload(torch, sw)
    for seg in (64, 1024):
        plan = batch.SplitPlan(sw.ln, sw.bf, DEV, segment_symbols=seg)
        out = split_launch(torch, dev, sw, plan, 14000, mstride=full, scratch=0xFF)
        check(torch, out, want, f"near ties: split seg {seg}", soft=K)
    uniform_control(torch, dev, sw, want, 14000, "near ties:")
    x, off, ln = dev
    out = poisoned_result(torch, sw.ln.size, sw.stride, full)
    d_bf = torch.from_numpy(sw.bf).to(DEV)
    res = batch.demod_batch(x, off, ln, d_bf, 14000, out=out, entry="mixed", diagnostics=True)
    assert res is out
    torch.cuda.synchronize()
    check(torch, out, want, "near ties: per-stream entry", soft=K)
