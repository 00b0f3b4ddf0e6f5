"""CPU only: the placement conditions of every input set of tests/test_gpu_clock_sweeps.py
(tests/clock_sweep_inputs.py) -- what those sweeps claim to cover is proved here without a GPU, from the oracle's
outputs and the numpy model of the totals: totals on and one below a bin edge, winners at every seam the kernels'
sources define, six wrong search rules each refuted at every rate, and a table of what geometry rules out that a rate
cannot leave quietly."""
import numpy as np
import pytest

from afskmodem_amd import batch
from oracle import afsk_oracle as O
from tests import clock_sweep_inputs as K
from tests import detect_model as DM
from tests import live_sweep_inputs as L
from tests import soft_cases as S
from tests import symbol_streams as G


def test_rates_are_the_sources_geometries_and_the_run_time_values():
    """Both lists are parsed from afsk_demod_impl.h: a geometry added there is swept, or fails here."""
    c = K.source_constants()
    assert len(c["fast"]) + len(c["gp"]) == 36 and len(set(c["fast"] + c["gp"])) == 36
    assert set(c["fast"] + c["gp"]) == set(batch.VALID_BIT_FRAMES) == set(S.ALL_BIT_FRAMES) - set(S.RT_BIT_FRAMES)
    assert len(K.rates()) == 46 and not set(K.RT_RATES) & set(K.compiled_rates())
    assert all(bf % 4 == 0 and 2 * bf < K.WINDOW for bf in K.rates())
    # the seam constants the placements are built from are the kernels' own
    assert (c["lanes_gc"], c["steps_gc"], c["step"], c["rt_gc"], c["rt_step"], c["lanes_max"]) == (72, 24, 1536, 24, 1536, 120)
    assert {K.form(bf) for bf in K.rates()} == {"lanes", "steps", "rt"}
    assert K.form(120) == "lanes" and K.form(128) == "steps" and K.form(124) == "rt"
    # the steps form divides by a magic multiplier while 65535 N^2 < 2^36 and in floating point above: both are swept
    magic = {65535 * (2 * bf) ** 2 < 1 << 36 for bf in K.rates() if K.form(bf) == "steps"}
    assert magic == {True, False} and K.WINDOW - 2 * 2044 == 8


def test_missing_table_is_what_the_inequalities_give():
    """MISSING equals the table recomputed from the geometry, and every rate's sweep holds exactly the other classes
    (check_rate asserts that per rate).  Nothing is missing up to bit_frames 640 but two pockets inside ONE lane's
    run, which N <= 64 alone allows; families A, D and the single pockets exist at all 46 rates."""
    assert K.MISSING == K.expected_missing()
    for cls, gone in K.MISSING.items():
        assert set(gone) <= set(K.rates())
        if cls != "B2_lane":
            assert all(bf > 640 for bf in gone), cls
    assert set(K.rates()) - set(K.MISSING["B2_lane"]) == {4, 8, 12, 16, 20, 24, 32}
    for bf in K.rates():
        have = {m["cls"] for m in K.sweep(bf).meta}
        assert {"A", "B1", "B_outside", "D"} <= have
        assert ("C" in have) == (bf <= 680) == ("B2_near" in have)


def test_rendered_cycles_are_the_oracles_tones():
    """The training cycle of tests/detect_model.py is mark ++ space of the oracle wherever a Receiver has the rate,
    and the local render equals symbol_streams.render there: the run-time rates get the same construction."""
    for bf in K.compiled_rates():
        t = G.tones(bf)
        assert np.array_equal(np.concatenate([t[1], t[0]]), DM.training_cycle(bf))
        assert np.array_equal(K.cycle(bf), O.training_cycle(48000 // bf))
    for bf in (28, 1028):
        t = K.tones(bf)
        assert np.array_equal(np.concatenate([t[1], t[0]]), DM.training_cycle(bf)) and t[0, 0] > 0 and t[1, 0] > 0
        x = K.render([1, 0, 1], bf, {0: (K.LEVEL, 0), 1: (K.LEVEL, -bf), 2: (K.LEVEL, bf + 1)}, 3)
        sym = x[3:].reshape(3, bf).astype(np.int64)
        assert not x[:3].any() and np.abs(sym).sum(axis=1).tolist() == [K.LEVEL * bf, K.LEVEL * bf - bf, K.LEVEL * bf + bf + 1]


def test_model_totals_are_the_literal_sums_on_sweep_streams():
    """detect_model.totals (running sums) against the literal definition on one stream of every family."""
    for bf in (4, 28, 100, 964, 2044):
        sw = K.sweep(bf)
        seen = set()
        for s, m in enumerate(sw.meta):
            if m["fam"] in seen:
                continue
            seen.add(m["fam"])
            x = K.window_of(sw, s)
            assert np.array_equal(DM.totals(x, bf), DM.totals_direct(x, bf)), (bf, m)
            assert K.total_at(x, bf, 0) == DM.totals(x, bf)[0]


@pytest.fixture(scope="module")
def whole():
    return K.load_all()


def test_model_first_minimum_is_the_oracles_clock_index(whole):
    sw, want = whole
    assert set(sw.bf.tolist()) == set(K.rates())
    assert (sw.ln >= K.WINDOW + 4 * sw.bf).all()
    K.check_model(sw, want)


@pytest.mark.parametrize("bf", K.rates())
def test_placements_and_refuted_rules(whole, bf):
    """Per rate: bump pairs on and below the edge, pockets at every seam and outside the search, pocket pairs, the
    attenuated transmissions' moving winner (and their payload), the top of the range -- and all six wrong rules
    refuted."""
    sw, want = whole
    killed = K.check_rate(sw, want, bf)
    assert set(killed) == set(K.WRONG_RULES) and min(killed.values()) > 0


def test_seams_lie_where_the_forms_hand_over():
    assert K.seams(40) == [72, 72 * 55] and -(-(4096 - 80) // 72) == 56
    assert K.seams(160) == [24, 1512, 1536, 3072]
    assert K.seams(100) == sorted({72, 72 * 54, 24, 1512, 1536, 3072}) and K.forms(100) == ("lanes", "rt")
    assert K.seams(2044) == [24, 1512] and K.placements(2044) == [0, 1, 6, 7]
    assert K.placements(40)[:5] == [0, 1, 71, 72, 73] and K.placements(40)[-2:] == [4014, 4015]


def test_live_rows_open_one_burst_at_block_quiet():
    """Family C at bit_frames 40 and 100 as live rows: the oracle's gate cuts one burst per row from block QUIET on,
    and the burst's clock index is the cycle each row was built for, with its payload decoded from there."""
    ls = K.live_set()
    want = L.expected(ls)
    K.check_live(ls, want)
