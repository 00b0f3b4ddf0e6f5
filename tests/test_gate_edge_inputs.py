"""The inputs of the gate edge tests (tests/gate_edge_inputs.py) are what they claim to be, and the CPU oracle's gate
over them agrees with the chunked Python model of the live walk (no GPU)."""
import numpy as np
import pytest

from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests import gate_edge_inputs as E
from tests.test_live_host import Model

BLOCK = E.BLOCK


@pytest.mark.parametrize("pair", E.PAIRS)
def test_six_block_sequences_hold_their_class_amplitudes_and_gate_like_the_model(pair):
    rows = E.live_rows(pair)
    seq = E.sequences()
    amps = np.array(E.class_amps(pair))
    assert rows.shape == (E.N_SEQ, 6 * BLOCK) and len({tuple(s) for s in seq.tolist()}) == E.N_SEQ
    s, e = pair
    assert {s, s + 1} <= set(amps.tolist()) and ({e - 1, e} <= set(amps.tolist()) or s == e)
    # exact block sums, all rows at once; the oracle's amplitude on a sample of them
    sums = np.abs(rows.astype(np.int64)).reshape(E.N_SEQ, 6, BLOCK).sum(axis=2)
    assert np.array_equal(sums, amps[seq] * BLOCK)
    for i in np.random.default_rng(1).choice(E.N_SEQ, 50, replace=False).tolist():
        assert [O.get_amplitude(rows[i, BLOCK * b: BLOCK * b + BLOCK]) for b in range(6)] == amps[seq[i]].tolist()
    want = E.expected_live(pair)
    got = []
    for c in range(E.N_SEQ):
        model = Model(lambda b: int(amps[seq[c, b]]), s, e)
        got += [(c, st, n, f) for T in (3000, 3000, 3000, 3000, 288) for st, n, f in model.push(T, flush=T == 288)]
    assert np.array_equal(np.array(got, np.int64), want)
    assert np.count_nonzero(want[:, 3] == _native.LIVE_OPEN_END) > 1000 and np.count_nonzero(want[:, 3] == 0) > 1000
    assert np.bincount(want[:, 0]).max() == 2                       # six blocks hold at most two bursts


def test_flat_captures_layout():
    flat, off, ln = E.flat_captures((18000, 14000))
    rows = E.live_rows((18000, 14000))
    assert (off % 2 == 0).any() and (off % 2 == 1).any()
    assert np.all(off[1:] - (off[:-1] + ln[:-1]) >= 0) and np.all(off[1:] - (off[:-1] + ln[:-1]) <= 2)
    assert np.all((ln[::3] > 6 * BLOCK) & (ln[::3] < 7 * BLOCK)) and np.all(ln[1::3] == 6 * BLOCK)
    for i in (0, 1, 2, 3, 7777, E.N_SEQ - 1):
        assert np.array_equal(flat[off[i]: off[i] + 6 * BLOCK], rows[i])
    nb, bs, bl, oe = E.expected_gate(flat[: off[300]], off[:300], ln[:300], (18000, 14000), 2)
    live = E.expected_live((18000, 14000))
    for i in range(300):                                            # a tail shorter than a block changes nothing
        mine = live[live[:, 0] == i]
        assert [(bs[i, k], bl[i, k]) for k in range(nb[i])] == [(r[1], r[2]) for r in mine]
        assert oe[i] == int(len(mine) > 0 and mine[-1, 3] == _native.LIVE_OPEN_END)


def test_every_sample_rows_are_decided_by_one_sample():
    rows = E.every_sample_rows()
    assert rows.shape == (2 * BLOCK, 3 * BLOCK)
    plain = E.square_rows(np.array([[0, 18000, 0], [0, 18001, 0]]))
    for p in range(BLOCK):
        up, down = rows[p].astype(np.int64), rows[BLOCK + p].astype(np.int64)
        assert np.nonzero(up != plain[0])[0].tolist() == [BLOCK + p] and abs(up[BLOCK + p]) == 18000 + 2048
        assert np.nonzero(down != plain[1])[0].tolist() == [BLOCK + p] and abs(down[BLOCK + p]) == 18000
        assert np.abs(up).sum() == BLOCK * 18001 and np.abs(down).sum() == BLOCK * 18001 - 1
    for p in (0, 1, 7, 8, 511, 512, 1023, 2046, 2047):
        assert O.get_amplitude(rows[p, BLOCK: 2 * BLOCK]) == 18001
        assert O.get_amplitude(rows[BLOCK + p, BLOCK: 2 * BLOCK]) == 18000
        assert O.gate_stream(rows[p], 18000, 14000, 4) == ([(BLOCK, 2 * BLOCK)], 0)
        assert O.gate_stream(rows[BLOCK + p], 18000, 14000, 4) == ([], 0)
