"""CPU only: the input sets of the transmit side's boundary sweeps (tests/tx_sweep_inputs.py).  Every ``check_*`` runs
here on the reference side alone -- what tests/test_gpu_tx_sweeps.py claims to cover is proved without a GPU --, the
numpy frame reference is held against the CPU oracle at every rate a Transmitter can have, and the constants the sets
rest on are tied to the kernels' source."""
import math

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from oracle import afsk_oracle as O
from tests import tx_sweep_inputs as X


def test_the_constants_the_sets_rest_on_are_the_sources():
    k = X.source_constants()
    assert k["kModChunk"] == k["kModThreads"] * 8 * k["kModIters"] == 16384 == X.BLOCK
    assert k["kTxTile"] == 4096 == X.TILE and k["kTxMinBlocks"] == 8192 == X.MIN_BLOCKS
    assert k["kWinBytes"] == 512
    assert k["kMixTile"] == 2048 and k["kMixMaxDegree"] == 32768
    # the tiles-per-block thresholds of the live pull: n * tiles >= 2 * and >= 4 * kTxMinBlocks
    assert X.TILES_N * 3 >= 2 * k["kTxMinBlocks"] > (X.TILES_N - 1) * 3 and X.TILES_N * 6 >= 4 * k["kTxMinBlocks"]
    assert -(-X.T2 // X.TILE) == 3 and -(-X.T4 // X.TILE) == 6 and X.TILES_N * 3 < 4 * k["kTxMinBlocks"]


@pytest.mark.parametrize("wav_quirk", [True, False], ids=["quirk", "ideal"])
def test_frames_ref_equals_the_oracle_at_all_48_rates(wav_quirk):
    assert len(X.RATES) == 48 and X.RATES[0] == 4 and X.RATES[-1] == 48000
    pay = X.seeded(77, 40)
    for bf in X.RATES:
        for plen, ts in ((0, 2), (1, 1), (40, 1), (1, 0)):
            n = X.tone_len(bf, ts, plen) + X.TAIL
            want = O.modulate_batch(np.frombuffer(pay, np.uint8)[None, :], [plen], [bf], [ts], [0], [n + 9], n + 9,
                                    wav_quirk)
            got = X.frames_ref(pay[:plen], bf, ts, wav_quirk)
            assert got.size == n and np.array_equal(got, want[:n]) and not want[n:].any(), (bf, plen, ts)
            # truncated and padded: the lengths the sets use
            for m in (1, bf - 1, 5 * bf + 3, n - 1, n + 9):
                assert np.array_equal(X.frames_ref(pay[:plen], bf, ts, wav_quirk, m), want[:m]), (bf, plen, ts, m)


def test_frames_ref_is_the_transmitters_wav_samples():
    for baud, tt in ((1200, 0.1), (6000, 0.02), (24, 0.0)):
        t = afskmodem.Transmitter(baud, tt)
        assert np.array_equal(X.frames_ref(b"hello", 48000 // baud, t.ts_cycles, True), t.wav_samples(b"hello"))


@pytest.mark.parametrize("name", list(X.MOD_SETS))
def test_modulator_sets(name):
    build, check = X.MOD_SETS[name]
    ms = build()
    check(ms)
    # the layout: no stream touches another, both parities of the first sample, a sample of sentinel either side
    assert (ms.off >= 1).all() and ms.off[-1] + ms.ln[-1] < ms.total
    assert (ms.off % 2 == 1).any() and (ms.off % 2 == 0).any()
    assert (ms.ln >= 1).all() and int(ms.ln.max()) < (1 << 30)


def test_set_a2_reaches_every_offset_the_formula_allows():
    """lim = bf * (2 ts + 4 + 14 plen) runs over the multiples of 2 bf from 4 bf on, so lim - 16384 k takes exactly the
    multiples of gcd(2 bf, 16384): computed here from the formula, and the builder must have realised every one of them
    in -16 ... 16 with the smallest k."""
    ms = X.set_a2()
    for bf, offsets in X.A2_OFFSETS.items():
        g = math.gcd(2 * bf, X.BLOCK)
        formula = {}
        for k in range(1, 2 * bf // g + 1):
            for o in offsets:
                if (X.BLOCK * k + o) % (2 * bf) == 0 and X.BLOCK * k + o >= 4 * bf:
                    formula.setdefault(o, k)
        assert sorted(formula) == [o for o in offsets if o % g == 0], bf
        assert formula == X.reachable_tone_ends(bf, offsets), bf
        built = {(m["o"], m["k"]) for m, b in zip(ms.meta, ms.bf) if b == bf}
        assert built == set(formula.items()), (bf, built, formula)
    # what the placement decides in the kernel, restated: the block that holds the tones' end, the blocks behind it
    lim, ln = ms.lim, ms.ln.astype(np.int64)
    last_block = (np.minimum(lim, ln) - 1) // X.BLOCK
    assert ((ln - 1) // X.BLOCK > last_block).any() and ((ln - 1) // X.BLOCK == last_block).any()
    assert (lim % X.BLOCK == 0).any() and (ln < lim).any() and (ln > lim).any() and (ln == lim).any()


@pytest.mark.parametrize("name", ["b1", "b2", "b3", "b4", "b5", "b6"])
def test_live_sets_place_every_feature(name):
    wavs = X.WavCache()
    specs = [X.live_spec(name, "uniform", (bf,)) for bf in X.LIVE_BFS]
    if name in ("b1", "b2"):
        specs.append(X.live_spec(name, "uniform", (48000,)))
    specs += [X.live_spec(name, "mixed"), X.live_spec(name, "rated")]
    for spec in specs:
        model, cols, _ = X.realise(spec, wavs.of(spec.table))
        X.check_live(spec, cols)
        assert [c.col for c in spec.chans] == cols.tolist()
        if name != "b5" or spec.kind == "uniform":                # (B5's rows are 256-byte messages: the uniform ones)
            X.check_rows(spec, model, cols, model.expected(spec.T))


def test_live_sets_for_several_tiles_per_block():
    for T in (X.T2, X.T4):
        for kind, bfs in (("uniform", (40,)), ("mixed", X.LIVE_BFS), ("rated", X.LIVE_BFS)):
            spec = X.live_spec("b1", kind, bfs, T)
            _, cols, _ = X.realise(spec)
            X.check_live(spec, cols)
            assert spec.n < X.TILES_N
    assert 4 * X.TILE in [c.col for c in X.live_spec("b1", "uniform", (40,), X.T4).chans]


def test_the_hold_form_starts_the_deferred_message_at_the_holdoff():
    table = [(bf, X.LIVE_TS[bf]) for bf in X.LIVE_BFS]
    wavs = X.WavCache()
    for d in X.HOLD_OFFSETS:
        model, _ = X.hold_case(table, d, wavs.of(table))
        n = len(table)
        out, pend, dfr = model.pull_hold(X.HOLD_FIRST, None, [1] * n, X.TILE + d, X.SENTINEL)
        assert not out.any() and (dfr == X.HOLD_FIRST).all() and (pend == 1).all()
        out, pend, dfr = model.pull_hold(X.T2, None, None, 0, X.SENTINEL)
        assert (dfr == X.TILE + d).all()
        for c in range(n):
            assert not out[c, : X.TILE + d].any() and out[c, X.TILE + d] in (X.HI, X.LO), (d, c)


def test_training_time_gives_the_ts_cycles_asked_for():
    for bf in X.RATES:
        for ts in (0, 1, 2, 3, 7, 2046):
            assert afskmodem.Transmitter(48000 // bf, X.training_time(bf, ts)).ts_cycles == ts, (bf, ts)
    assert X.training_time(4, 0) == 0.0


def test_noise_streams_cover_every_tail():
    ns = X.noise_set()
    assert (ns.off % 2 == 1).all()
    lens = sorted(set(ns.ln.tolist()))
    assert lens == sorted(set(list(range(1, 18)) + [2048 * k + d for k in (1, 2) for d in range(-9, 10)]))
    combos = {(int(s), r) for s, r in zip(ns.scale, ns.rail)}
    assert combos == {(s, r) for s in (0, 1, 1 << 24, (1 << 31) - 1) for r in (False, True)}
    for ln in lens:
        assert {(int(s), r) for s, r, n in zip(ns.scale, ns.rail, ns.ln) if n == ln} == combos
    for base in X.NOISE_BASES:
        want = X.noise_reference(ns, base)
        untouched = np.ones(ns.total, bool)
        for o, n in zip(ns.off, ns.ln):
            untouched[o: o + n] = False
        assert (want[untouched] == ns.clean[untouched]).all()
        zero = ns.scale == 0
        for o, n in zip(ns.off[zero], ns.ln[zero]):
            assert np.array_equal(want[o: o + n], ns.clean[o: o + n])
        assert (want != ns.clean).any()
    # where both run, the oracle and the numpy restatement of the generator agree
    row = ns.clean[ns.off[-1]: ns.off[-1] + ns.ln[-1]]
    assert np.array_equal(O.add_noise(row, X.NOISE_SEED, 5, 1 << 24), X.M.noise_direct(row, X.NOISE_SEED, 5, 1 << 24, 0))
