"""CPU suite of tests/soft_cases.py, the helper of tests/test_gpu_soft_large.py: the prototype streams meet the
conditions the GPU cases rely on (asserted on the oracle's rows), the footprint checker accepts a correct result and
rejects every kind of wrong one it exists for, and the GPU cases' stream counts lie on the intended side of the
thresholds in afsk_demod_ring.h -- a moved threshold fails here instead of silently un-arming a GPU case."""
import numpy as np
import pytest

from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests import soft_cases as S


@pytest.mark.parametrize("bf", S.ALL_BIT_FRAMES)
def test_prototype_conditions_hold_for_every_rate(bf):
    """Both parities of the clock index, three or more prototypes with corrections (the forced ones among them, 4
    codewords each with the payload unchanged), a payload beyond one 64-byte flush for bit_frames <= 20; the base
    set's streams are capped, and the margin rows are wide enough for every symbol there is."""
    ps = S.prototypes(bf)
    S.assert_conditions(ps)
    w = ps.want
    assert len(ps.streams) == 48 + 3 + (bf <= S.FLUSH_MAX_BIT_FRAMES)
    assert (ps.lens[:48] <= S.PROTO_CAP).all() and (ps.bf == bf).all()
    assert (w["corrected"][ps.forced] == 4).all() and (w["nbytes"][ps.forced] == 5).all()
    assert (w["bytes"][ps.forced, :5] == w["bytes"][ps.forced[0], :5]).all() and (w["status"][ps.forced] == 0).all()
    ci = w["clock_idx"]
    assert (ci >= 0).all() and len({(2 * int(c)) & 15 for c in ci}) >= 7
    K = S.symbols_in(ps.lens, ci, ps.bf)
    assert (w["n_symbols"] <= K).all() and int(K.max()) + 8 <= ps.margin_stride
    assert int(w["nbytes"].max()) <= S.OUT_STRIDE
    assert S.prototypes(bf) is ps                                      # computed once


def test_mixed_set_has_every_ring_shift_and_the_refusal_model_is_the_oracles():
    ps = S.merged(S.MIXED_BIT_FRAMES)
    S.assert_conditions(ps, mixed=True)
    assert len(ps.streams) == sum(len(S.prototypes(b).streams) for b in S.MIXED_BIT_FRAMES)
    la = S.build_launch(ps, S.N_MIXED[0], 11, invalid_bf=True)
    n = S.N_MIXED[0]
    assert la.lens.size == n and abs(int(la.refused.sum()) - n / 9) < 2          # about one slot in nine
    r = np.nonzero(la.refused)[0]
    assert not la.refused[r - 1].any() and not la.refused[r[:-1] + 1].any()      # between decoded ones
    assert set(la.lens[r]) >= set(S.REFUSED_LENGTHS) and set(la.bf[r]) >= set(S.REFUSED_BIT_FRAMES)
    assert sorted(set(la.want["status"][r])) == [_native.ST_TOO_SHORT, _native.ST_INVALID_BAUD, _native.ST_BAD_LENGTH]
    # every copy carries its prototype's row
    ok = np.nonzero(~la.refused)[0][:500]
    for j in ok[:50]:
        x = la.flat[la.off[j]: la.off[j] + la.lens[j]]
        i = next(i for i in np.nonzero(ps.lens == la.lens[j])[0] if np.array_equal(ps.streams[i][: la.lens[j]], x))
        assert la.want["corrected"][j] == ps.want["corrected"][i] and la.want["nbits"][j] == ps.want["nbits"][i]
        assert np.array_equal(la.want["margins"][j], ps.want["margins"][i])
    assert (la.off % 8 == 0).all()
    # the refusal row is what the oracle answers where it accepts the input at all (lengths 0 and 4095)
    for length in (0, 4095):
        j = r[la.lens[r] == length][0]
        w = O.demod_batch_soft(la.flat, la.off[j: j + 1], [length], la.bf[j: j + 1], 14000, out_stride=S.OUT_STRIDE,
                               margin_stride=8)
        for f in S.INT_FIELDS + ("corrected", "n_symbols"):
            assert int(w[f][0]) == int(la.want[f][j]), (length, f)


# ---------------------------------------------------------------------------------------------- the checker
def model_result(launch, out_stride, margin_stride):
    """A guarded result holding exactly what a correct kernel writes for ``launch``."""
    import torch
    n = launch.lens.size
    res = S.guarded_result(n, out_stride, margin_stride, "cpu")
    w = launch.want
    for f in S.INT_FIELDS + ("corrected",):
        getattr(res, f).copy_(torch.from_numpy(w[f]))
    for s in range(n):
        nb = min(int(w["nbytes"][s]), out_stride)
        res.bytes[s, :nb] = torch.from_numpy(w["bytes"][s, :nb].copy())
        ns = min(int(w["n_symbols"][s]), margin_stride)
        res.margins[s, :ns] = torch.from_numpy(w["margins"][s, :ns].copy())
    return res


@pytest.fixture(scope="module")
def small_launch():
    return S.build_launch(S.merged((40, 8, 1000, 136)), None, 0, invalid_bf=True)


def _decoded(launch, min_symbols=40):
    return int(np.nonzero(~launch.refused & (launch.want["n_symbols"] >= min_symbols) & (launch.want["nbytes"] > 0))[0][3])


def _refused(launch):
    return int(np.nonzero(launch.refused)[0][2])


MUTATIONS = {
    "wrong margin at n_symbols - 1": lambda r, la: r.margins[_decoded(la), int(la.want["n_symbols"][_decoded(la)]) - 1].add_(1),
    "spill into a refused stream's margin row": lambda r, la: r.margins[_refused(la), 0].fill_(17),
    "byte changed at nbytes": lambda r, la: r.bytes[_decoded(la), int(la.want["nbytes"][_decoded(la)])].fill_(0),
    "int32 guard element changed": lambda r, la: r.guards.ints["nbits"][7].fill_(0),
    "int32 guard element behind changed": lambda r, la: r.guards.ints["status"][la.lens.size + 8].fill_(0),
    "byte guard row changed": lambda r, la: r.guards.bytes[la.lens.size + 1, 0].fill_(0),
    "margin guard row changed": lambda r, la: r.guards.margins[0, -1].fill_(0),
    "corrected non-zero on a refused stream": lambda r, la: r.corrected[_refused(la)].fill_(4),
    "corrected left stale on a refused stream": lambda r, la: r.corrected[_refused(la)].fill_(S.INT_SENTINEL),
    "margin written at K": lambda r, la: r.margins[_decoded(la), int(S.symbols_in(la.lens, la.want["clock_idx"], la.bf)[_decoded(la)])].fill_(5),
    "status of a refused stream": lambda r, la: r.status[_refused(la)].fill_(0),
    "payload byte": lambda r, la: r.bytes[_decoded(la), 0].add_(1),
}


def test_checker_accepts_a_correct_result(small_launch):
    la = small_launch
    assert la.refused.sum() >= 15 and la.lens.size <= S.N_SMALL_MAX
    res = model_result(la, S.OUT_STRIDE, la.margin_stride)
    S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=True)
    S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=False)
    # truncating strides: nbytes and n_symbols still report the full counts
    res = model_result(la, S.NARROW_OUT_STRIDE, S.NARROW_MARGIN_STRIDE)
    assert (la.want["nbytes"] > S.NARROW_OUT_STRIDE).any() and (la.want["n_symbols"] > S.NARROW_MARGIN_STRIDE).any()
    S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=True)


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_checker_rejects(small_launch, name):
    la = small_launch
    res = model_result(la, S.OUT_STRIDE, la.margin_stride)
    MUTATIONS[name](res, la)
    with pytest.raises(AssertionError):
        S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=True)


def test_split_path_check_lets_segments_fill_their_own_row(small_launch):
    """one_wave=False: an entry between n_symbols and the row end is the segment's business; a refused row, a guard
    row and the symbols the reference demodulated are still checked."""
    la = small_launch
    res = model_result(la, S.OUT_STRIDE, la.margin_stride)
    res.margins[_decoded(la), la.margin_stride - 1] = 5
    S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=False)
    with pytest.raises(AssertionError):
        S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=True)
    res.margins[_refused(la), 3] = 5
    with pytest.raises(AssertionError):
        S.check_footprint(res, res.guards, la.want, la.lens, la.bf, one_wave=False)


def test_refuse_rewrites_every_second_stream():
    ps = S.prototypes(40)
    first = S.build_launch(ps, None, 0, refused_every=0)
    assert not first.refused.any() and (first.want["corrected"][ps.forced] > 0).all()
    second = S.refuse(first, np.arange(1, first.lens.size, 2), S.REFUSED_LENGTHS)
    assert second.refused[1::2].all() and not second.refused[0::2].any()
    assert (second.want["corrected"][1::2] == 0).all() and (second.want["clock_idx"][1::2] == -1).all()
    assert (second.host_lens == first.lens).all() and not first.refused.any()       # the first launch is unchanged
    assert second.refused[ps.forced].any() and not second.refused[ps.forced].all()


# ---------------------------------------------------------------------------------------------- thresholds
def test_launch_sizes_lie_on_the_intended_side_of_the_source_thresholds():
    t = S.source_thresholds()
    hint, grouped, uniform = t["kHintMinStreams"], t["kHintMinStreamsGrouped"], t["kHintMinStreamsUniform"]
    short4, short8, warm = t["kHintMinStreamsShort4"], t["kHintMinStreamsShort8"], t["kWarmMinStreams"]
    lo, hi = S.N_MIXED
    assert hint <= lo < warm, "mixed entry, first size: the hint alone"
    assert hi >= max(hint, warm), "mixed entry, second size: hint and warming"
    lo, hi = S.N_GROUPED
    assert grouped <= lo < min(hint, warm), "grouped entry, first size: armed for the grouped walk and not for the mixed one"
    assert hi >= max(grouped, warm)
    assert S.N_UNIFORM >= max(uniform, short4, warm), "uniform entry: the large form of every bit_frames but 8"
    assert S.N_UNIFORM < short8 <= S.N_UNIFORM_BF8 and S.N_UNIFORM_BF8 >= warm, "uniform entry, bit_frames 8"
    assert uniform <= S.N_HINT_ONLY < warm and not {4, 8} & set(S.HINT_ONLY_BIT_FRAMES)
    assert S.N_SMALL_MAX < min(t.values()), "the small forms"
    small = sum(len(S.prototypes(b).streams) for b in (40, 8, 1000, 136))
    assert small <= S.N_SMALL_MAX
    # the rates: every compile-time geometry of the kernels, and two bit_frames without one
    assert len(set(S.ALL_BIT_FRAMES)) == 38 and len(set(S.MIXED_BIT_FRAMES)) == 32
    from afskmodem_amd import batch
    assert set(S.ALL_BIT_FRAMES) - set(S.RT_BIT_FRAMES) == set(batch.VALID_BIT_FRAMES) and len(batch.VALID_BIT_FRAMES) == 36
    assert all(b % 4 == 0 and 48000 % b for b in S.RT_BIT_FRAMES)
