"""CPU only: the symbol-level generator (tests/symbol_streams.py) against the oracle, and the placement conditions
of every input set of tests/test_gpu_split_sweeps.py (tests/split_sweep_inputs.py) -- what those sweeps claim to
cover is proved here without a GPU, from the oracle's outputs alone."""
import numpy as np
import pytest

from oracle import afsk_oracle as O
from tests import split_sweep_inputs as I
from tests import symbol_streams as G


def _one(x, bf, amp_end=14000):
    w = O.demod_batch(x, [0], [len(x)], [bf], amp_end, out_stride=256)
    return {k: v[0] for k, v in w.items()}


def test_render_levels_and_lead():
    for bf in (8, 40, 100, 2000):
        x = G.render([1, 0, 1, 1], bf, {1: (14000, -1), 2: (0, 0), 3: (9000, 1)}, lead=3)
        assert x.dtype == np.int16 and len(x) == 3 + 4 * bf and not x[:3].any()
        sym = x[3:].reshape(4, bf).astype(np.int64)
        assert (sym[0] == O.mark_tone(48000 // bf)).all()
        assert np.abs(sym[1]).sum() == 14000 * bf - 1 and (np.sign(sym[1]) == np.sign(O.space_tone(48000 // bf))).all()
        assert not sym[2].any()
        assert np.abs(sym[3]).sum() == 9000 * bf + 1 and sym[3][0] == 9001
        assert O.get_amplitude(sym[1]) == 13999 and O.get_amplitude(sym[3]) == 9000


def test_coded_bits_are_the_transmitters():
    data = bytes(range(256))
    for bf in (8, 40):
        want = O.get_frames(data, 48000 // bf, 0.5)
        c = int(48000 // bf * 0.5 / 2)
        got = G.render(G.training(c) + G.coded(data), bf)
        assert (want[: len(got)] == got).all() and not want[len(got):].any()
    assert G.flip([0, 1, 1], [0, 2]) == [1, 1, 0]


@pytest.mark.parametrize("bf", [8, 40, 100, 2000])
def test_placement_every_lead_in(bf):
    """clock_idx == lead, term_frame == lead + len(training) * bf, nbits == len(data) with silence behind."""
    data = G.coded(b"\x5a\xc3\x0f")
    for lead in range(16):
        for even in (False, True):
            for c in ((1, 3) if bf == 2000 else (30, 60) + ((2047,) if lead in (0, 1, 3, 5, 7, 10) else ())):
                train = G.training(c, even)
                w = _one(G.stream(train, data, bf, lead=lead), bf)
                assert (w["clock_idx"], w["term_frame"], w["nbits"]) == (lead, lead + len(train) * bf, len(data)), \
                    (lead, even, c)
                assert bytes(w["bytes"][:3]) == b"\x5a\xc3\x0f"


@pytest.mark.parametrize("bf", [8, 40, 100])
@pytest.mark.parametrize("amp_end", [14000, 9000])
def test_threshold_symbol(bf, amp_end):
    """One below the threshold stops the decode there; on it and one above do not."""
    data = G.coded(bytes(range(10)))
    train = G.training(20)
    for j in (0, 1, 19, 20, 64):
        for d, want in ((-1, j), (0, len(data)), (1, len(data))):
            w = _one(G.stream(train, data, bf, lead=2, level={j: (amp_end, d)}), bf, amp_end)
            assert w["nbits"] == want and w["clock_idx"] == 2, (j, d)


def test_terminator_index_builder():
    for kt in range(3, 300):
        t = G.training_ending_at(kt)
        assert len(t) == kt + 1 and t[-4:] == [1, 0, 0, 0]
        hits = [k for k in range(3, len(t)) if t[k - 3: k + 1] == [1, 0, 0, 0]]
        assert hits == [kt]


def test_sweep_a_alignment_forms():
    sw = I.sweep_a()
    I.check_a(sw, I.oracle(sw))


@pytest.mark.parametrize("straddle", [False, True])
def test_sweep_b_end_of_stream(straddle):
    sw = I.sweep_b(straddle)
    I.check_b(sw, I.oracle(sw), straddle)


def test_sweep_c_terminator_positions():
    sw = I.sweep_c()
    I.check_c(sw, I.oracle(sw))


@pytest.mark.parametrize("amp_end", I.D_AMP_ENDS)
def test_sweep_d_squelch_stops(amp_end):
    sw = I.sweep_d(amp_end)
    I.check_d(sw, I.oracle(sw, amp_end))


def test_sweep_e_byte_pack_and_corrections():
    sw = I.sweep_e()
    I.check_e(sw, I.oracle(sw, soft=int((sw.ln // sw.bf).max()) + 8))


def test_sweep_f_shortened_lengths():
    sw, short, longest, refused = I.sweep_f()
    I.check_f(sw, short, longest, refused, I.oracle(sw, ln=short))
