"""GPU parity (-m gpu) -- the auto receiver's rate decision (afsk_live_auto.hip: ``rate_score``'s one signed pass with
lane-stepped phases and one division, ``decide``'s minimum of (score << 6) | position, the winner packed into
StreamDemod::spare across pushes, ``max_score``) on bursts where that arithmetic decides something: every candidate
alone on transmissions, noise, full-scale and offset windows (S), scores on and one past a bin edge that d(ci) does
not show (E), the clock index on both sides of every offset where the cycle count drops (N), ties of part of the list
and candidates one count apart (T), and the largest scores and rates through seeded push sizes (P).

The inputs come from tests/auto_sweep_inputs.py; every expected value is tests/live_auto_model.py's -- the oracle's
gate, tests/detect_model.py on the burst's first 4096 samples, the oracle's demod at the rate named --, never the
generator's intent and never another GPU path's.  Each test first asserts, from the oracle's gate, that every burst
starts where it was built, and the placements tests/test_auto_sweep_inputs_host.py proves on the CPU, on the very rows
it compares.  Result buffers are poisoned before the first push; unused slots must read bit_frames 0 and rate_score -1
after every push.  Integer path: tolerance zero."""
import numpy as np
import pytest

from afskmodem_amd import _native
from afskmodem_amd.live import LiveReceiver
from tests import auto_sweep_inputs as A
from tests import detect_model as D
from tests.gpu_common import torch_cuda  # noqa: F401  (fixture)
from tests.live_drive import collect, push_sizes
from tests.test_gpu_split_sweeps import BYTE_POISON, I32_POISON

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 8192                                    # the whole sweep's push size
# one-candidate receivers by rate group: about two thousand channels a test at the most
GROUPS = ((4,), (8, 12), (16, 20, 24, 32), (40, 48, 60, 64, 80, 96, 100, 120),
          (128, 160, 192, 200, 240, 300, 320, 384, 400, 480, 500, 600, 640, 800, 960, 1000, 1200, 1500, 1600, 1920, 2000))
RAGGED = (0, 1, 7, 2047, 2048, 2049, 5000, T)


def receiver(aset, chunk=T, pairs=None, **kw):
    start, end = ([p[0] for p in pairs], [p[1] for p in pairs]) if pairs else A.PAIR
    return LiveReceiver(aset.n, "auto", start, end, candidates=aset.candidates, max_burst_len=None, max_chunk_len=chunk,
                        device=DEV, **kw)


def poisoned(rx):
    """A result of the receiver's with poison in every output a push writes per slot."""
    out = rx.alloc_result()
    out.demod.flat.fill_(BYTE_POISON)
    for t in (out.n_closed, out.burst_start, out.burst_len, out.flags, out.bit_frames, out.rate_score):
        t.fill_(I32_POISON)
    return out


def gather(out, got):
    """One push's bursts, and every unused slot cleared."""
    nc = out.n_closed.cpu().numpy()
    assert ((nc >= 0) & (nc <= out.slots)).all()
    bf, sc = out.bit_frames.cpu().numpy(), out.rate_score.cpu().numpy()
    unused = np.arange(out.slots)[None, :] >= nc[:, None]
    assert not bf[unused].any() and (sc[unused] == -1).all(), "unused slots must read bit_frames 0 and rate_score -1"
    collect(out, got)


def run(torch, aset, sizes=None, each=None, **kw):
    """The set through one receiver in pushes of ``sizes`` and a flush; the bursts per channel."""
    d = torch.from_numpy(aset.host.copy()).to(DEV)
    sizes = sizes or push_sizes(T, aset.host.shape[1])
    rx = receiver(aset, max(sizes), **kw)
    out = poisoned(rx)
    got = [[] for _ in range(aset.n)]
    p = 0
    for t in sizes + [None]:
        if t is None:
            rx.flush(out=out)
        else:
            rx.push(d[:, p: p + t], out=out)
            p += t
        gather(out, got)
        if each:
            each(out)
    assert p == aset.host.shape[1]
    rx.close()
    return got


def compare(aset, got, want, tag):
    """Whole rows, every key the expected rows have; then rate, score and clock index against the detector's model on
    the window cut from the host capture at the reported start."""
    for c in range(aset.n):
        assert len(got[c]) == len(want[c]), (tag, c, aset.meta[c])
        for g, w in zip(got[c], want[c]):
            for k, v in w.items():
                assert g[k] == v, (tag, c, aset.meta[c], k, g[k], v)
            if w["status"] != _native.ST_INVALID_BAUD:
                det = D.detect(aset.host[c, g["start"]: g["start"] + A.WINDOW], aset.candidates)
                assert (g["bit_frames"], g["rate_score"], g["clock_idx"]) == \
                    (det["bit_frames"], det["score"], det["clock_idx"]), (tag, c, aset.meta[c])


# ------------------------------------------------------------------------------------------------ S, E, N, T alone

@pytest.mark.parametrize("rates", GROUPS, ids=lambda g: f"{g[0]}_to_{g[-1]}")
def test_every_candidate_alone(torch_cuda, rates):
    """candidates=[bf], one receiver per rate, the plain untapped cell: families S, E, N and T of the rate -- every
    candidate's own score is the reported one, at every lane step 64 mod 2bf and every quarter width."""
    assert sorted(r for g in GROUPS for r in g) == list(A.RATES)
    for bf in rates:
        aset = A.rate_set(bf)
        want = A.expected(aset)
        A.check_rate(aset, want)
        compare(aset, run(torch_cuda, aset), want, f"candidates [{bf}]")


# ------------------------------------------------------------------------------------------------ E, all 36

def test_bin_edge_under_all_candidates_and_max_score_on_the_edge(torch_cuda):
    """Family E under the whole list: 12767 and 12768 at the tile's rate.  Then max_score = 12767 in a tapped
    receiver: score == max_score decodes as before, score == max_score + 1 is refused -- INVALID_BAUD, bit_frames 0,
    the score kept, clock_idx and term_frame -1, no tap bytes."""
    aset = A.full_list_e()
    want, refused = A.expected(aset), A.expected(aset, A.MAX_SCORE)
    A.check_full_list_e(aset, want, refused)
    compare(aset, run(torch_cuda, aset), want, "E, all 36 candidates")
    tapped = np.zeros(aset.n, np.int64)

    def each(out):
        tapped[:] += out.tap.n.cpu().numpy()
    got = run(torch_cuda, aset, each=each, max_score=A.MAX_SCORE, progressive=True)
    compare(aset, got, refused, "E, all 36 candidates, max_score on the edge")
    past = np.array([m["side"] == "past" for m in aset.meta])
    assert not tapped[past].any() and tapped[~past].tolist() == [w[0]["nbytes"] for w, p in zip(want, past) if not p]
    assert tapped.any()


# ------------------------------------------------------------------------------------------------ T

def test_ties_of_part_of_the_list_and_one_count_between_neighbours(torch_cuda):
    """Every neighbouring pair of rates as [b, a] and as [a, b]: nobody lower, a alone lower by one count (it wins
    from position 1), both lower (position 0 wins).  Then all 36 in descending order: the winner deep in the list with
    a tie behind it."""
    for a, b, p in A.t_pairs():
        for order in ((b, a), (a, b)):
            aset = A.pair_set(a, b, p, order)
            want = A.expected(aset)
            A.check_pair(aset, want)
            compare(aset, run(torch_cuda, aset), want, f"candidates {list(order)}")
    aset = A.descending_set()
    want = A.expected(aset)
    A.check_descending(aset, want)
    compare(aset, run(torch_cuda, aset), want, "all 36 descending")


# ------------------------------------------------------------------------------------------------ P

P_SEEDS = (9501, 9504, 9509)


def test_packed_rate_and_score_survive_the_pushes(torch_cuda):
    """The largest scores and the largest bit_frames in pushes drawn from {1, 7, 2047, 2048, 2049, 8192}: the deciding
    block -- the burst's second -- ends a push, lies inside one, and comes in a later push than the burst's first; the
    burst is reported pushes later with the rate and the score unchanged."""
    decided = (A.QUIET + 2) * A.B                              # samples pushed when the window is complete
    where = set()
    for seed in P_SEEDS:
        rng = np.random.default_rng(seed)
        for aset in A.p_sets():
            want = A.expected(aset)
            A.check_gate(aset, want)
            sizes = push_sizes("random", aset.host.shape[1], rng, A.P_STEPS)
            ends = np.cumsum(sizes)
            where.add("end" if decided in ends else "inside")
            where.add("later" if ((ends > A.QUIET * A.B) & (ends < decided)).any() else "same")
            assert len(sizes) < 200
            compare(aset, run(torch_cuda, aset, sizes), want, f"P, candidates {aset.candidates}, seed {seed}")
    assert {"end", "inside", "later"} <= where


# ------------------------------------------------------------------------------------------------ the other cells

def ragged(torch, aset, seed):
    """Every channel takes its own number of samples per push (device lengths, 0 included; loud garbage beyond a
    length), then one flush."""
    n, total = aset.host.shape
    rng = np.random.default_rng(seed)
    d = torch.from_numpy(aset.host.copy()).to(DEV)
    rx = receiver(aset)
    out = poisoned(rx)
    got = [[] for _ in range(n)]
    pos = np.zeros(n, np.int64)
    cols = torch.arange(T, device=DEV)[None, :]
    zero_seen = False
    while pos.min() < total:
        lens = np.minimum(rng.choice(RAGGED, n), total - pos).astype(np.int32)
        zero_seen |= bool(((lens == 0) & (pos < total)).any())
        rows = torch.gather(d, 1, (torch.from_numpy(pos).to(DEV)[:, None] + cols).clamp(max=total - 1))
        lens_d = torch.from_numpy(lens).to(DEV)
        buf = torch.where(cols < lens_d[:, None], rows, torch.full_like(rows, 12345))
        rx.push(buf, out=out, lengths=lens_d)
        gather(out, got)
        pos += lens
    assert zero_seen
    rx.flush(out=out)
    gather(out, got)
    rx.close()
    return got


@pytest.mark.parametrize("cell", ["tapped", "ragged", "per_channel"])
def test_reduced_rows_through_the_other_cells(torch_cuda, cell):
    """The rule: per family the row of largest expected score (the first on a tie) at bit_frames 40 and at 1000 -- the
    two forms of the sink's clock search, 1000 the largest rate that has every family -- under the rate's own list and,
    together, under all 36 candidates.  Through the tapped cell, the ragged cell (device lengths, a zero length
    included) and the cell with a threshold pair per channel."""
    for aset in A.cell_sets():
        pairs = [A.PAIRS[c % 2] for c in range(aset.n)] if cell == "per_channel" else None
        want = A.expected(aset, pairs=pairs)
        A.check_gate(aset, want)
        if cell == "tapped":
            got = run(torch_cuda, aset, progressive=True)
        elif cell == "ragged":
            got = ragged(torch_cuda, aset, 9600)
        else:
            got = run(torch_cuda, aset, pairs=pairs)
        compare(aset, got, want, f"{cell} cell, candidates {aset.candidates}")
