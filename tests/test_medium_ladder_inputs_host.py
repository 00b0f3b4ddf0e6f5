"""CPU proof of the live medium's edge matrix (tests/medium_ladder_inputs.py): every reachable (consumer, class, offset)
was placed, the three timeline models agree wherever more than one can express a case, and the inputs would catch a
subtly wrong kernel -- shown without running one, by running the TRUE model on deliberately altered tables or inputs and
requiring that the rows built for the edge concerned come out different, at every offset 1 ... 7 of its class.  These
are conditions on the inputs; tests/test_gpu_medium_ladder.py compares the kernels on the very same sets."""
import numpy as np
import pytest

from tests import live_delay_model as D
from tests import live_fade_model as FD
from tests import live_fir_model as F
from tests import live_mix_model as M
from tests import medium_ladder_inputs as L

SMALL = [n for n in L.base_names() if n.startswith("small")]
SMALL8 = [n for n in SMALL if n.startswith("small-h8-")]


def test_the_classifier_on_groups_worked_out_by_hand():
    g = L.group_class
    assert g(8, 8, 0, 8) == L.SILENT and g(0, 8, 5, 8) == L.SRC and g(16, 23, 0, 8) == ("EDGE", None, 7, None)
    assert g(-8, 24, 8, 8) == L.RING and g(-8, 24, 11, 8) == ("EDGE", None, None, 5)      # slots 3 ... 7, then 0 ... 2
    assert g(-3, 24, 16, 16) == ("EDGE", 3, None, None) and g(-3, 1, 16, 16) == ("EDGE", 3, 4, None)
    assert g(-3, 0, 16, 16) == ("EDGE", 3, 3, None) and g(-5, 24, 3, 16) == ("EDGE", 5, None, 2)
    assert g(-5, 24, 5, 16) == ("EDGE", 5, None, None)            # the ring's end coincides with column 0: not inside
    assert L.class_key(("EDGE", 5, None, 2)) == ("ZERO_RING", 5, 2) and L.class_key(("EDGE", None, 7, None)) == ("EDGE_LEN", 7)
    b = L.fir_block(2048, 2000, 16, 100, 4096)
    assert (b["base"], b["Kp"], b["full"], b["skip"]) == (33, 16, True, False)
    b = L.fir_block(2048, 5000, 17, 33, 4096)                     # the delay clamped to hist_len - 16
    assert (b["d"], b["base"], b["Kp"], b["full"], b["skip"]) == (4080, -2048, 32, False, False)
    assert L.fir_block(0, 0, 1, 0, 8)["skip"] and L.fir_block(0, 3, 300, 9, 16)["K"] == 17
    k = L.knot_boundary
    assert k(16, 3, 4) == (0, "inner") and k(29, 3, 4) == (3, "end") and k(29, 3, 8) == (3, "inner")
    assert k(L.WRAP - 5, 3, 4) == (5, "wrap") and k(17, 5, 4) == (None, None) and k(L.WRAP + 61, 3, 1) == (3, "end")
    h = L.history_class
    assert h(16, 24, 24, 8, 8) == ("ONE_SRC",) and h(16, 24, 9, 8, 8) == ("ONE_ZERO",)
    assert h(16, 24, 23, 8, 8) == ("HEDGE", None, 7, None) and h(16, 24, 24, 11, 8) == ("HEDGE", None, None, 5)
    assert h(0, 7, 7, 8, 8) == ("HEDGE", 7, None, None) and h(0, 1, 1, 7, 8) == ("HEDGE", 1, None, None)
    assert (L.THREADS, L.TILE, L.CHUNK, L.MAX_TAPS, L.MIN_SHIFT) == (256, 2048, 16, 256, 3)


def test_every_reachable_consumer_class_and_offset_was_placed():
    cases = L.all_cases()
    got = L.check_ladder(cases)
    assert len(L.required()) >= 300 and all(r in got for r in L.required())
    # the matrix is the issue's: both small rings at every residue and before 2^32, the lengths, every delay, every K
    for h in L.SMALL_HIST:
        assert L.small_starts(h)[:h] == tuple(range(h)) and L.WRAP - 5 in L.small_starts(h)
        case = L.CASES[f"small-h{h}-p0"]
        assert case.hist_len == h and case.ticks[:2] == (24, 24) and {1, 7} <= set(case.ticks)
        assert case.lens[1] == (-3, 0, 1, 7, 8, 9, 23, 24, 29)
        want = {(s, d, K, f) for s in range(9) for d in range(h + 1) for f in (False, True)
                for K in (None, 1, 2, 3, 8, 9, 15, 16, 17) if K is None or d + K - 1 <= h}
        assert {(m["s"], m["d"], m["K"], m["faded"]) for m in case.meta} == want and len(case.meta) == len(want)
        assert np.diff(case.tables()["row_ptr"]).tolist() == [1] * case.n_out
    tile = L.CASES["tile"]
    assert tile.hist_len == 4096 and set(tile.ticks) == {2048 + 24} and any(tile.noise)
    assert {len(h) for h in tile.filters} == {16, 17, 255, 256} and max(c.n_out for c in cases) <= 2000
    assert sorted(np.diff(L.CASES["rows"].tables()["row_ptr"]).tolist()) == [0, 2, 2, 2, 5, 5]
    assert {x[2] for x in L.CASES["rows"].links} >= {L.U, -L.U, 65535, 0}
    # every rung is reached from below: a case of rung r runs on the media r ... 3
    assert {c.rung for c in cases} == {0, 1, 2, 3}


def test_an_unreachable_entry_that_was_placed_fails_the_check(monkeypatch):
    cases = [L.CASES[n] for n in L.ladder_names("rows")]
    monkeypatch.setattr(L, "required", lambda: [])
    L.check_ladder(cases)
    monkeypatch.setitem(L.UNREACHABLE, (5, ("skip", False)), "not so")
    with pytest.raises(AssertionError):
        L.check_ladder(cases)


@pytest.mark.parametrize("base", L.base_names())
def test_the_three_models_agree_where_more_than_one_expresses_a_case(base):
    """The fade model over ``link_fade`` all -1 is the fir model on every case of rung <= 2 and, the filters unnamed
    too, the delay model on rung <= 1; at rung 0 it is the plain model.  A restriction's rows are its case's."""
    top = L.CASES[base]
    full = L.expected(base)[0]
    for name in L.ladder_names(base):
        case = L.CASES[name]
        rows, rings, poss = L.expected(name)
        assert poss == [case.position(t + 1) for t in range(len(case.ticks))]
        if case.rung <= 2:
            assert (case.tables()["link_fade"] == -1).all()
            fir = L.run_model(case, timeline=F.Timeline)
            assert all((a == b).all() for a, b in zip(rows, fir[0])) and all((a == b).all() for a, b in zip(rings, fir[1]))
        if case.rung <= 1:
            assert (case.tables()["link_filter"] == -1).all()
            delay = L.run_model(case, timeline=D.Timeline)
            assert all((a == b).all() for a, b in zip(rows, delay[0]))
        if case.rung == 0:
            t = case.tables()
            for tick, T in enumerate(case.ticks):
                plain = M.mix(L.sources(case, tick), t["row_ptr"], t["link_src"], t["link_gain_q15"], case.n_out, T,
                              src_lens=list(case.lens[tick]), noise_scale_q24=np.array(case.noise), seed=case.seed,
                              noise_idx_base=3, pos=case.position(tick))
                assert (plain == rows[tick]).all()
        if case is not top and not any(top.noise):                # (noise is keyed by the row's index)
            kept = [x[0] for x in top.links if L.link_rung(x) <= case.rung]
            assert len(kept) == case.n_out and all((full[t][kept] == rows[t]).all() for t in range(len(rows)))
    # the ring is the sources, not a product of the tables: poison never enters it, the last column of a tick is there
    rows, rings, _ = L.expected(base)
    for tick, T in enumerate(top.ticks):
        src = L.sources(top, tick)
        slot = (top.position(tick) + T - 1) & (top.hist_len - 1)
        for s in range(top.n_src):
            assert rings[tick][s, slot] == (src[s, T - 1] if top.length(tick, s) == T else 0)
            assert (src[s, top.length(tick, s):] == L.POISON).all() and src.shape[1] == T + 3


def test_every_edge_has_a_row_that_is_heard():
    """Of the rows built for an edge class of a part, at least one is not all zeros in its tick."""
    heard = {}
    for case in L.all_cases():
        rows = L.expected(case.name)[0]
        for (part, fact), where in L.placements(case).items():
            if part != "H" and fact[0] == "class":
                heard[(part, fact)] = heard.get((part, fact), False) or any(rows[t][r].any() for t, r in where)
    assert len(heard) > 150 and all(heard.values()), [k for k, v in heard.items() if not v]


# ------------------------------------------------------------------------------------------------------ alterations

def differing(case, altered, part_facts):
    """{fact: True} for the facts of ``part_facts`` that have a row, placed for them, whose altered expectation differs
    from the true one in the tick it was placed in."""
    true = L.expected(case.name)[0] if case.name in L.CASES else L.run_model(case)[0]
    found = set()
    for (part, fact), where in L.placements(case).items():
        if (part, fact) in part_facts and any((true[t][r] != altered[t][r]).any() for t, r in where):
            found.add((part, fact))
    return found


def every_offset(parts, name):
    return {(p, ("class", (name, o))) for p in parts for o in L.OFFSETS}


def test_alteration_lengths_ignored_lets_the_poison_through():
    want = every_offset(("U", "UF", "S1"), "EDGE_LEN") | {("U", ("class", L.SILENT)), ("UF", ("class", L.SILENT))}
    found = set()
    for base in SMALL:
        for rung in (1, 2) if base in SMALL8 else (1,):
            case = L.CASES[f"{base}/r{rung}"]
            found |= differing(case, L.run_model(case, src_lens=None)[0], want)
    for base in SMALL8:                                           # the faded unfiltered links: fir_group_edge's decision
        top = L.CASES[base]
        case = L.subset(top, [x[0] for x in top.links if x[4] is None and x[5] is not None], "faded")
        found |= differing(case, L.run_model(case, src_lens=None)[0], want)
    assert found == want, sorted(want - found, key=str)


def test_alteration_a_delay_clamped_to_hist_len_minus_one():
    want = every_offset(("U",), "EDGE_RING") | {("U", ("class", L.RING))}
    found = set()
    for base in SMALL:
        case = L.CASES[f"{base}/r1"]
        rows = [x[0] for x, m in zip(case.links, case.meta) if m["d"] == case.hist_len]
        only = L.subset(case, rows, "longest")                    # the rows at delay hist_len alone
        assert only.n_out == 9 and all(x[3] == case.hist_len for x in only.links)
        t = only.tables()
        t["link_delay"] = np.minimum(t["link_delay"], case.hist_len - 1)
        found |= differing(only, L.run_model(only, tables=t)[0], want)
    assert found == want, sorted(want - found, key=str)


def test_alteration_h0_dropped_where_the_taps_fill_their_last_chunk():
    """The K == Kp tail word carries h[0] alone: without it every K % 16 == 0 filter loses its first tap."""
    tile = L.CASES["tile"]
    rows = [x[0] for x in tile.links if x[4] is not None and len(tile.filters[x[4]]) % L.CHUNK == 0]
    case = L.subset(tile, rows, "full")
    t = case.tables()
    for f, h in enumerate(case.filters):
        assert h[0] != 0
        if len(h) % L.CHUNK == 0:
            t["filter_taps"][t["filter_ptr"][f]] = 0
    altered = L.run_model(case, tables=t)[0]
    want = every_offset(("S1", "S2", "S1f", "S2f"), "EDGE_ZERO") | {("S1", ("full", True)), ("S2f", ("full", True))}
    found = differing(case, altered, want)
    assert found == want, sorted(want - found, key=str)
    small = L.CASES["small-h16-p3/r2"]                            # and the K = 16 rows of a small ring
    t = small.tables()
    t["filter_taps"][t["filter_ptr"][L.SMALL_KS.index(16)]] = 0
    altered = L.run_model(small, tables=t)[0]
    true = L.expected(small.name)[0]
    for x, m in zip(small.links, small.meta):
        assert (m["K"] == 16) == any((a[x[0]] != b[x[0]]).any() for a, b in zip(true, altered)), m


def test_alteration_the_ring_read_runs_into_the_next_sources_ring():
    """Columns before 0 come from the NEXT source row (the last one's from the first): what a read past the ring's end
    returns on the device, where the rings lie back to back."""
    want = every_offset(("U",), "EDGE_RING") | every_offset(("U",), "EDGE_ZERO") | {("U", ("class", L.RING))}
    found = set()
    for base in SMALL:
        case = L.CASES[f"{base}/r1"]
        sent = []

        def swap(tl, tick, case=case, sent=sent):
            if tick:
                cur = np.zeros((case.n_src, case.ticks[tick - 1]), np.int16)
                src = L.sources(case, tick - 1)
                for s in range(case.n_src):
                    cur[s, :case.length(tick - 1, s)] = src[s, :case.length(tick - 1, s)]
                sent.append(cur)
                tl.X = np.roll(np.concatenate(sent, axis=1), -1, axis=0)
        found |= differing(case, L.run_model(case, before_tick=swap)[0], want)
    assert found == want, sorted(want - found, key=str)


def first_pair_envelope(knots, p, u):
    """``FD.envelope`` with the knot pair of a group's FIRST column kept for all 8 (the groups begin at column 0)."""
    knots = np.asarray(knots, np.int64)
    L_ = knots.size
    u = np.asarray(u, np.int64) & 0xFFFFFFFF
    first = u[(np.arange(u.size) // 8) * 8]
    n = (first >> p) & (L_ - 1)
    m = (n + 1) & (L_ - 1)
    q = u & ((1 << p) - 1)                                        # (what fade_env8 gives with its ``next`` always false)
    return knots[n] + (((knots[m] - knots[n]) * q) >> p)


def test_alteration_the_first_knot_pair_kept_for_all_8_columns(monkeypatch):
    want = {(p, ("knot", col)) for p in ("UF", "S1f") for col in range(1, 8)}
    found = set()
    for base in SMALL8:
        top = L.CASES[base]
        case = L.subset(top, [x[0] for x in top.links if x[5] == 1], "track1")      # the L = 4 track's links
        true = L.run_model(case)[0]
        with monkeypatch.context() as mp:
            mp.setattr(FD, "envelope", first_pair_envelope)
            altered = L.run_model(case)[0]
        for (part, fact), where in L.placements(case).items():
            if (part, fact) in want and any((true[t][r] != altered[t][r]).any() for t, r in where):
                found.add((part, fact))
    assert found == want, sorted(want - found, key=str)
    u = np.arange(40, 64)
    assert (first_pair_envelope([7, 7, 7, 7], 3, u) == 7).all()
    assert (first_pair_envelope([0, 800, 0, 0], 3, u)[:8] == FD.envelope([0, 800, 0, 0], 3, u)[:8]).all()


def test_alteration_the_envelope_offset_saturated_and_why_modulo_2_31_cannot_show():
    """An offset cut to 2^31 - 1, as a signed conversion would, is heard.  One taken modulo 2^31 is not, by arithmetic
    (``UNREACHABLE``): every track's period divides 2^31 -- asserted here on the rows themselves, so that a track
    format that changes this turns the entry into a requirement."""
    top = L.CASES[f"small-h8-p{L.WRAP - 29}"]
    high = [x[0] for x in top.links if x[5] is not None and x[6] >= 1 << 31]
    case = L.subset(top, high, "high-offsets")
    assert case.n_out >= 50 and {x[5] for x in case.links} == {0, 1}
    true = L.run_model(case)[0]
    t = case.tables()
    t["link_fade_offset"] = np.minimum(t["link_fade_offset"], (1 << 31) - 1)
    cut = L.run_model(case, tables=t)[0]
    heard = {x[5] for x in case.links if any((a[x[0]] != b[x[0]]).any() for a, b in zip(true, cut))}
    assert heard == {1}                                           # (track 0 is one knot: it has no position to lose)
    t["link_fade_offset"] = case.tables()["link_fade_offset"] & ((1 << 31) - 1)
    assert (t["link_fade_offset"] != case.tables()["link_fade_offset"]).all()
    folded = L.run_model(case, tables=t)[0]
    assert all((a == b).all() for a, b in zip(true, folded)) and "offset mod 2^31" in L.UNREACHABLE
    assert all((len(k) * per) <= 1 << 31 and (1 << 31) % (len(k) * per) == 0 for k, per in case.fades)
