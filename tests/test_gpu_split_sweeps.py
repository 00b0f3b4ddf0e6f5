"""GPU parity (-m gpu) -- systematic sweeps of the sequence-parallel path's boundaries (afsk_split.hip): the eight
alignment forms of the 1200-baud stage B in every prefetch regime, the end of the stream at every bit of a bitmap
word, the terminator and the squelch stop at every position around word, segment and 64-word loop edges (symbols
exactly on the squelch threshold included), bytes packed across words, and a plan relaunched over poisoned scratch
and with shorter device lengths.

The inputs come from tests/split_sweep_inputs.py; every expected value is the CPU oracle's, never the generator's
intent and never another GPU path's.  Each sweep first asserts, from the oracle's outputs, that the placement it was
built for happened (the same conditions tests/test_symbol_streams_host.py proves on the CPU).  Every launch writes
into poisoned outputs: bytes past nbytes must come back untouched.  Every batch also goes once through the uniform
entry, one launch per rate: a failure there separates a generator surprise from a split bug.  Integer path:
tolerance zero."""
import numpy as np
import pytest

from afskmodem_amd import _native, batch
from tests import split_sweep_inputs as I
from tests.gpu_common import assert_same, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BYTE_POISON = 0xA5
I32_POISON = -1515870811                     # 0xA5A5A5A5
MARGIN_POISON = 0x7A7A7A7A
MARGIN_GUARD = 64


def upload(torch, sw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return t(sw.flat), t(sw.off), t(sw.ln)


def poisoned_result(torch, n, stride, mstride=None):
    """Outputs whose every byte is poison; with ``mstride`` also corrected and a margins array with a guard behind."""
    out = batch.alloc_result(n, stride, DEV)
    out.flat.fill_(BYTE_POISON)
    if mstride is not None:
        out.corrected = torch.full((n,), I32_POISON, dtype=torch.int32, device=DEV)
        out.margin_store = torch.full((n * mstride + MARGIN_GUARD,), MARGIN_POISON, dtype=torch.int32, device=DEV)
        out.margins = out.margin_store[: n * mstride].view(n, mstride)
    return out


def check(torch, out, want, tag, soft=None):
    """Every field against the oracle; row bytes past nbytes still poison.  ``soft`` = (K per stream): also corrected,
    the margins of the symbols the reference demodulated, and poison from symbol K on and behind the array."""
    got = out.cpu()
    assert_same(got, want, tag)
    stride = got.bytes.shape[1]
    assert (want["nbytes"] <= stride).all(), tag
    past = np.arange(stride)[None, :] >= want["nbytes"][:, None]
    bad = np.nonzero(((got.bytes != BYTE_POISON) & past).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: bytes past nbytes written in streams {bad[:5]}"
    if soft is None:
        return
    K = soft
    corr, marg = out.corrected.cpu().numpy(), out.margins.cpu().numpy()
    assert corr.tolist() == want["corrected"].tolist(), tag
    mstride = marg.shape[1]
    for s in range(marg.shape[0]):
        k = min(int(want["n_symbols"][s]), mstride)
        assert marg[s, :k].tolist() == want["margins"][s, :k].tolist(), (tag, s)
        assert (marg[s, max(int(K[s]), 0):] == MARGIN_POISON).all(), (tag, s)
    assert (out.margin_store[-MARGIN_GUARD:].cpu().numpy() == MARGIN_POISON).all(), tag


def split_launch(torch, dev, sw, plan, amp_end, d_ln=None, mstride=None, scratch=None):
    x, off, ln = dev
    if scratch is not None:
        plan.scratch.fill_(scratch)
    out = poisoned_result(torch, sw.ln.size, sw.stride, mstride)
    res = batch.demod_batch_split(x, off, ln if d_ln is None else d_ln, plan, amp_end, out=out,
                                  diagnostics=mstride is not None)
    assert res is out
    torch.cuda.synchronize()
    return out


def split_sweep(torch, sw, want, segments, amp_end=14000, tag=""):
    """``sw`` through the split path once per segment size (scratch poisoned), then once through the uniform entry."""
    dev = upload(torch, sw)
    for seg in segments:
        plan = batch.SplitPlan(sw.ln, sw.bf, DEV, segment_symbols=seg)
        out = split_launch(torch, dev, sw, plan, amp_end, scratch=0xFF)
        check(torch, out, want, f"{tag} split seg {seg} amp_end {amp_end}")
    uniform_control(torch, dev, sw, want, amp_end, tag)


def uniform_control(torch, dev, sw, want, amp_end, tag):
    """The same batch through the default kernels: ``batch.demod_batch(..., entry="uniform")``, one launch per rate."""
    x, off, ln = dev
    for bf in sorted(set(sw.bf.tolist())):
        idx = np.nonzero(sw.bf == bf)[0]
        d_idx = torch.from_numpy(idx).to(DEV)
        out = poisoned_result(torch, idx.size, sw.stride)
        batch.demod_batch(x, off[d_idx].contiguous(), ln[d_idx].contiguous(), int(bf), amp_end, out=out,
                          entry="uniform")
        torch.cuda.synchronize()
        check(torch, out, {k: v[idx] for k, v in want.items()}, f"{tag} CONTROL uniform bit_frames {bf} amp_end {amp_end}")


def test_alignment_forms_times_pass_counts(torch_cuda):
    """(a) bit_frames 40: all eight compile-time forms (ci & 7) at even and at odd stream offsets, the first segment
    with 1, 2, 3, 4, 5 and more passes: every vmcnt wait of the four-slot ring and its refill in every form."""
    sw = I.sweep_a()
    want = I.oracle(sw)
    I.check_a(sw, want)
    split_sweep(torch_cuda, sw, want, I.A_SEGMENTS, tag="(a)")


@pytest.mark.parametrize("straddle", [False, True], ids=["past_terminator", "around_1024"])
def test_end_of_stream_at_every_bit_of_a_word(torch_cuda, straddle):
    """(b) K = (len - ci - 1) // bf over 64 consecutive values per rate (40, 8, 100, 2000) and lead-in, and the lengths
    around one K; around symbol 1024 with the default segment: a partial last pass, and a stream ending on the edge."""
    sw = I.sweep_b(straddle)
    want = I.oracle(sw)
    I.check_b(sw, want, straddle)
    split_sweep(torch_cuda, sw, want, (64, 128, 1024) if straddle else (64, 128), tag="(b)")


def test_terminator_at_every_position(torch_cuda):
    """(c) the terminator's last symbol at every index in [60, 200] (both parities, every straddle of a word edge)
    and in [4090, 4102] (the 64-word search step of stage C), and a data-like 1,0,0,0 inside the training."""
    sw = I.sweep_c()
    want = I.oracle(sw)
    I.check_c(sw, want)
    split_sweep(torch_cuda, sw, want, I.C_SEGMENTS, tag="(c)")


@pytest.mark.parametrize("amp_end", I.D_AMP_ENDS)
def test_squelch_stop_at_every_position(torch_cuda, amp_end):
    """(d) the first quiet data symbol at every position 0 ... 140 -- silent, one below the threshold, and exactly
    on it (which does not stop) --, at the last symbol K - 1, never, and around the stop search's second trip."""
    sw = I.sweep_d(amp_end)
    want = I.oracle(sw, amp_end)
    I.check_d(sw, want)
    split_sweep(torch_cuda, sw, want, I.D_SEGMENTS, amp_end, tag="(d)")


def test_byte_pack_across_words_corrected_and_margin_cut(torch_cuda):
    """(e) 96-byte payloads from an even and an odd first data symbol: bytes whose 14 coded bits lie across a word,
    single flipped bits in every third codeword, two codewords with two (the oracle says what comes out); margins
    with a row longer than the stream and with one cut at first + 100, inside a segment."""
    torch = torch_cuda
    sw = I.sweep_e()
    full = int((sw.ln // sw.bf).max()) + 8
    dev = upload(torch, sw)
    want = I.oracle(sw, soft=full)
    K = I.check_e(sw, want)
    for mstride in (full, None):
        if mstride is None:
            ci, first, _ = I.geometry(sw, want)
            mstride = int(first.min()) + 100
            assert (mstride < want["n_symbols"]).all() and mstride % I.E_SEGMENTS[0]
        else:
            assert (K < mstride).all()
        for seg in I.E_SEGMENTS:
            plan = batch.SplitPlan(sw.ln, sw.bf, DEV, segment_symbols=seg)
            out = split_launch(torch, dev, sw, plan, 14000, mstride=mstride, scratch=0xFF)
            check(torch, out, want, f"(e) seg {seg} margin_stride {mstride}", soft=K)
    uniform_control(torch, dev, sw, want, 14000, "(e)")


def test_scratch_and_plan_reuse(torch_cuda):
    """(f) one plan, five launches over the same samples: scratch 0xFF, scratch 0x00, scratch as left behind, device
    lengths shortened stream by stream (whole trailing segments dropped, two streams below 4096: TOO_SHORT), and the
    full lengths again.  Every launch against the oracle at the lengths it was given, into poisoned outputs."""
    torch = torch_cuda
    sw, short, longest, refused = I.sweep_f()
    mstride = 96
    want = I.oracle(sw, soft=mstride)
    want_short = I.oracle(sw, ln=short, soft=mstride)
    I.check_f(sw, short, longest, refused, want_short)
    K = I.geometry(sw, want)[2]
    K_short = np.where(want_short["status"] == _native.ST_TOO_SHORT, 0, I.geometry(sw, want_short, short)[2])
    dev = upload(torch, sw)
    d_short = torch.from_numpy(short).to(DEV)
    plan = batch.SplitPlan(sw.ln, sw.bf, DEV, segment_symbols=I.F_SEGMENT)
    for n, (scratch, d_ln, w, k) in enumerate([(0xFF, None, want, K), (0x00, None, want, K), (None, None, want, K),
                                               (0xFF, d_short, want_short, K_short), (None, None, want, K)], 1):
        out = split_launch(torch, dev, sw, plan, 14000, d_ln=d_ln, mstride=mstride, scratch=scratch)
        check(torch, out, w, f"(f) launch {n}", soft=k)
    uniform_control(torch, dev, sw, want, 14000, "(f)")
