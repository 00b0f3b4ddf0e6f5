"""CPU only: the placement conditions of every input set of tests/test_gpu_auto_sweeps.py
(tests/auto_sweep_inputs.py) -- what those sweeps claim to cover is proved here without a GPU, from the oracle's gate,
the detector's model (tests/detect_model.py) and the auto receiver's model (tests/live_auto_model.py): every clock
index, cycle count and bin side, which candidates tie, the device's one-pass form of the score restated in numpy and
held to the model on every window, seven wrong forms each refuted at every rate that has the family, and a table of
what geometry rules out that a rate cannot leave quietly."""
import numpy as np
import pytest

from afskmodem_amd import batch
from tests import auto_sweep_inputs as A
from tests import detect_model as D
from tests import symbol_streams as G

# rows per one-candidate set (families S, E, N, T of the rate), summed over the 36 rates; DESIGN 8.12.1 repeats these
ALONE_STREAMS = 7628
OTHER_STREAMS = {"E, all 36": 62, "T, pair lists": 204, "T, descending": 5, "cells": 16, "P": 39}


def test_rates_are_the_receivers_and_the_table_is_what_the_inequalities_give():
    """MISSING equals the table recomputed from the geometry: E and N at the five rates that count one cycle at
    every clock index (N > 2047), T nowhere -- position 4094 reaches the eight rates position 4000 does not."""
    assert A.RATES == tuple(batch.VALID_BIT_FRAMES) and len(A.RATES) == 36
    assert A.MISSING == A.expected_missing()
    assert A.MISSING["E"] == tuple(bf for bf in A.RATES if 2 * bf > 2047) == A.MISSING["N"]
    assert [bf for bf in A.RATES if A.t_pos(bf) == A.T_POS_FAST] == [4, 8, 12, 16, 20, 24, 32, 40]
    for bf in A.RATES:
        assert A.n_of(bf, A.t_pos(bf) - 2 * bf + 1) == 1 and 0 <= A.t_pos(bf) - 2 * bf + 1 < A.WINDOW - 2 * bf
        if bf in A.MISSING["E"]:
            assert all(A.n_of(bf, ci) == 1 for ci in range(A.WINDOW - 2 * bf))
        else:
            assert A.n_of(bf, 0) >= 2 and A.n_of(bf, A.WINDOW - 2 * bf - 1) == 1
    assert {len(A.families_of(bf)) for bf in A.RATES} == {2, 4}


def test_square_symbols_are_the_oracles_tones_and_the_tile_is_the_training_cycle():
    for bf in A.RATES:
        t = G.tones(bf)
        assert np.array_equal(A.square(bf, [0, 1]), np.concatenate([t[0], t[1]]))
        assert np.array_equal(A.square(bf, [1, 0]), D.training_cycle(bf))
        x = A.tile_stream(bf, 3, {1: 5}).astype(np.int64)
        assert (x[:3] == A.LEVEL).all() and x[3 + 2 * bf] == A.LEVEL - 5
        x[3 + 2 * bf] = A.LEVEL
        assert np.array_equal(x[3: 3 + 4 * bf], np.tile(A.cycle(bf, A.LEVEL), 2))
    assert A.square(2, [1, 0]).tolist() == [D.HI, D.HI, D.HI, D.LO] and len(A.square(4000, [1])) == 4000


@pytest.mark.parametrize("bf", A.RATES)
def test_lane_phases_in_closed_form_are_the_stepped_ones(bf):
    """The phase a lane reaches by adding 64 mod N and subtracting N once is (j mod N) for sample j -- at every rate,
    over the longest pass the rate has, and so is the closed form ``kernel_score`` uses."""
    total = A.n_of(bf, 0) * 2 * bf
    stepped = A.lane_phases_stepped(bf, total)
    assert np.array_equal(stepped, A.lane_phases(bf, total))
    assert np.array_equal(stepped, np.arange(total) % (2 * bf))
    assert (64 % (2 * bf) != 0) == (bf not in (4, 8, 16, 32))


@pytest.mark.parametrize("bf", A.RATES)
def test_placements_and_refuted_forms(bf):
    """Per rate, candidates=[bf]: the gate cuts every burst where it was built; every family's placement; the device's
    form equals the model's score on every window; and the six wrong scores each differ on at least one stream -- the
    two that need more than one counted cycle wherever families E and N exist."""
    aset = A.rate_set(bf)
    want = A.expected(aset)
    A.check_rate(aset, want)
    assert aset.n == A.rows_alone(bf)
    killed = A.check_forms(aset)
    for f in A.FORMS:
        if f in A.N_FORMS and bf in A.MISSING["E"]:
            assert killed[f] == 0, (bf, f)                      # score = d(ci) by definition: nothing to refute
        else:
            assert killed[f] > 0, (bf, f, killed)
    # the refutations do not rest on family S alone: E refutes the rounded mean and d(ci), N both wrong counts
    if "E" in A.families_of(bf):
        e = A.check_forms(A.subset(aset, aset.rows(fam="E")))
        n = A.check_forms(A.subset(aset, aset.rows(fam="N")))
        assert e["rounded"] > 0 and e["d_ci"] > 0 and n["n_more"] > 0 and n["n_fewer"] > 0, (bf, e, n)


def test_stream_count():
    assert sum(A.rows_alone(bf) for bf in A.RATES) == ALONE_STREAMS
    cells = A.cell_sets()
    alone, pool = A.p_sets()
    pairs = sum(A.pair_set(a, b, p, (a, b)).n for a, b, p in A.t_pairs()) * 2
    assert {"E, all 36": A.full_list_e().n, "T, pair lists": pairs, "T, descending": A.descending_set().n,
            "cells": sum(s.n for s in cells), "P": alone.n + pool.n} == OTHER_STREAMS


def test_full_list_names_the_tiles_rate_on_both_sides_of_the_bin_and_max_score_separates_them():
    """Family E under all 36 candidates: the tile's rate wins at clock index 0 with 12767 / 12768, the runner-up at
    least 1000 away; at max_score = 12767 the first burst of every pair is what it was, the second is refused."""
    aset = A.full_list_e()
    want = A.expected(aset)
    refused = A.expected(aset, A.MAX_SCORE)
    A.check_full_list_e(aset, want, refused)
    assert {w[0]["rate_score"] for w in want} == {A.MAX_SCORE, A.MAX_SCORE + 1}
    assert any(w[0]["nbytes"] == 2 for w in want)              # (where the payload fits: a burst that decodes)


def test_pairs_tie_and_split_by_one_count_and_the_last_candidate_would_win_differently():
    """Every neighbouring pair in both orders: no candidate lower (position 0), a alone lower (it wins from position
    1 in [b, a]), both lower (position 0).  ``decide`` with the positions reversed answers differently on every tie:
    refuted for all 36 rates."""
    seen = set()
    for a, b, p in A.t_pairs():
        for order in ((b, a), (a, b)):
            aset = A.pair_set(a, b, p, order)
            scores = A.check_pair(aset, A.expected(aset))
            assert [A.decide(s) for s in scores] == [0, order.index(a), 0]
            assert [A.decide(s, last_wins=True) for s in scores] == [1, order.index(a), 1]
            seen |= {a, b}
    assert seen == set(A.RATES)


def test_descending_list_has_its_winner_deep_with_a_tie_behind():
    aset = A.descending_set()
    want = A.expected(aset)
    A.check_descending(aset, want)
    for c in range(aset.n):
        s = D.detect(aset.window(c), aset.candidates)["scores"]
        assert aset.candidates[A.decide(s)] == want[c][0]["bit_frames"]
        assert (A.decide(s, last_wins=True) != A.decide(s))


def test_reduced_rows_and_the_rows_of_largest_score_and_rate():
    """The reduced rows open one burst at block QUIET under both pairs of the per-channel cell; the P rows hold the
    largest rate and scores above 2^15 (alone) and above 28000 (under all 36 candidates)."""
    sets = A.cell_sets()
    assert [s.candidates for s in sets] == [(40,), (1000,), None]
    for s in sets:
        assert [m["fam"] for m in s.meta] == list(A.FAMILIES) * (s.n // 4)
        A.check_gate(s, A.expected(s))
        A.check_gate(s, A.expected(s, pairs=[A.PAIRS[c % 2] for c in range(s.n)]))
    alone, pool = A.p_sets()
    for s in (alone, pool):
        want = A.expected(s)
        A.check_gate(s, want)
        got = [A.detected(s, want, c) for c in range(s.n)]
        assert max(g[0] for g in got) == 2000
        assert max(g[1] for g in got) > (1 << 15 if s is alone else 28000)
