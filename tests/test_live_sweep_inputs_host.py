"""CPU only: the input sets of the streaming receiver's boundary sweeps (tests/live_sweep_inputs.py).  Every
``check_*`` runs on the oracle's outputs -- what tests/test_gpu_live_sweeps.py claims to cover is proved here without a
GPU --, and every row goes block by block through the model of the streaming sink (tests/live_stream_model.py), which
must equal the oracle field for field: the placement proof and a model check in one."""
import numpy as np
import pytest

from tests import live_sweep_inputs as L
from tests.live_stream_model import demod_streaming


def model_equals_oracle(ls, want, rows=None):
    for c in range(ls.n) if rows is None else rows:
        w = want[c][0]
        burst = ls.host[c, w["start"]: w["start"] + w["len"]]
        got = demod_streaming(burst, int(ls.bf[c]), int(ls.a_end[c]), max_payload_len=ls.maxp)
        for f in L.FIELDS + ("corrected", "bytes"):
            assert got[f] == w[f], (c, int(ls.bf[c]), f, got[f], w[f])


def test_set_a_block_edge_inside_a_symbol():
    ls, want = L.load("a")
    L.check_a(ls, want)
    model_equals_oracle(ls, want)


def test_set_b_terminator_at_every_position():
    ls, want = L.load("b")
    L.check_b(ls, want)
    model_equals_oracle(ls, want)


@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_set_c_squelch_stop_at_every_position(far):
    ls, want = L.load("c_far" if far else "c")
    L.check_c(ls, want, far)
    # (the model walks every symbol in Python: of the far rows, every third)
    model_equals_oracle(ls, want, range(0, ls.n, 3) if far else None)


def test_set_d_hamming_and_byte_carry():
    ls, want = L.load("d")
    L.check_d(ls, want)
    model_equals_oracle(ls, want)


def test_set_e_near_tie_decisions():
    ls, want = L.load("e")
    found = L.check_e(ls, want)
    # bit_frames 8 has every class but the one its geometry cannot reach
    assert [k for k in L.E_CLASSES if found[8][k] == 0] == list(L.E_MISSING[8])
    model_equals_oracle(ls, want)


def test_symbol_classes():
    assert L.symbol_class(80, 81, 40) == "lt_same_quotient" and L.symbol_class(79, 81, 40) == "lt_other_quotient"
    assert L.symbol_class(80, 80, 40) == "tie" and L.symbol_class(119, 80, 40) == "gt_within_bf"
    assert L.symbol_class(120, 80, 40) == "gt_beyond_bf"
    for bf in (8, 40, 2000):
        for bit in (0, 1):
            M, S = L.symbol_sums(L.G.tones(bf)[bit], bf)
            assert (M, S)[1 - bit] == 0 and (M, S)[bit] == 65535 * bf // 2


def test_thin_mix_keeps_every_kind_of_row():
    ls, want = L.load("mix")
    assert set(ls.bf.tolist()) == {8, 40, 100} and set(ls.a_end.tolist()) == {14000, 9000}
    for key in ("on_edge", "false", "every_word", "extra"):
        assert (ls.col(key, 0) > 0).any(), key
    assert len(set(np.diff(ls.bf).tolist())) > 2               # interleaved, not sorted by rate
    L.geometry(ls, want)
    assert ls.host.shape[1] <= 50 * L.B
    far, want = L.load("mix_far")
    assert (far.col("far", 0) > 0).sum() == L.set_c(True).n and set(far.bf.tolist()) == {8, 40, 100}
    L.geometry(far, want)
