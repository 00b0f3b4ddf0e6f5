"""The rate detector without a GPU: the numpy model of its definition (tests/detect_model.py) tied to the reference's
recorded clock indices and to the CPU oracle, the accuracy list on the model, and the argument checks of
``batch.detect_rates``, ``modem.detect_baud`` and ``modem.load_batch_auto`` that need no device."""
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, modem
from oracle import afsk_oracle as O
from tests import detect_model as M
from tests.golden_inputs import build_input


def test_valid_bit_frames_are_the_36_values_a_receiver_accepts():
    assert list(batch.VALID_BIT_FRAMES) == M.VALID_BIT_FRAMES == sorted(M.VALID_BIT_FRAMES)
    assert len(batch.VALID_BIT_FRAMES) == _native.DETECT_MAX_CANDIDATES == 36
    batch.validate_bit_frames(batch.VALID_BIT_FRAMES)
    for bf in range(1, 2100):
        ok = True
        try:
            batch.validate_bit_frames(bf)
        except Exception:
            ok = False
        assert ok == (bf in batch.VALID_BIT_FRAMES), bf


def test_the_header_declares_the_entry_and_the_binding_mirrors_it():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "afsk_amd.h")).read()
    params = re.search(r"^extern int afsk_detect_rate_batch\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params.split(",")]
    res, args = _native.DETECT_SIGNATURES["afsk_detect_rate_batch"]
    assert len(kinds) == len(args) == 12
    assert [k for k in kinds if k != "ptr"] == ["int32_t", "int32_t"] and kinds[3] == kinds[5] == "int32_t"
    assert re.search(r"#define AFSK_DETECT_MAX_CANDIDATES 36\b", hdr)
    assert hasattr(_native.lib(), "afsk_detect_rate_batch")


def test_running_sums_equal_the_literal_definition():
    rng = np.random.default_rng(5)
    for x in (rng.integers(-32768, 32768, 4200).astype(np.int16), np.full(4096, -32768, np.int16),
              np.full(4096, 32767, np.int16)):
        for bf in (4, 40, 300, 2000):
            assert np.array_equal(M.totals(x, bf), M.totals_direct(x, bf)), bf
            assert M.totals(x, bf).max() < 1 << 28


def test_model_clock_index_equals_the_reference_on_the_golden_cases(golden):
    """(a) every recorded decode case with a clock index and at least 4096 samples, at its own rate."""
    seen = 0
    for c in golden["decode_cases"]:
        if c["clock_idx"] < 0 or c["n_samples"] < M.WINDOW:
            continue
        x = build_input(c)
        assert len(x) == c["n_samples"]
        assert M.candidate(x, 48000 // c["baud"])[1] == c["clock_idx"], c["tag"]
        seen += 1
    assert seen > 100


def test_model_clock_index_and_minimum_equal_the_oracle():
    """(b) seeded inputs: noise, and noisy transmissions behind a lead-in."""
    rng = np.random.default_rng(77)
    for k, bf in enumerate((4, 8, 20, 40, 96, 160, 500, 1000, 2000)):
        baud = 48000 // bf
        noise = rng.integers(-32768, 32768, 4096 + 16 * k).astype(np.int16)
        sig = np.concatenate([np.zeros(int(rng.integers(0, 2048)), np.int16),
                              afskmodem.Transmitter(baud, 0.2).frames(b"oracle")])
        sig = M.add_noise(np.concatenate([sig, np.zeros(M.WINDOW, np.int16)]), 6.0, rng)
        for x in (noise, sig):
            _, ci, d = M.candidate(x, bf)
            assert ci == O.recover_clock_index(x, baud), bf
            assert d == O.get_diff(O.training_cycle(baud), x[ci: ci + 2 * bf]), bf


def test_model_names_the_true_rate_on_the_whole_accuracy_list():
    """(c) every rate with bf <= 1000, clean / 10 dB / 5 dB, all 36 candidates: no case left out."""
    cases = M.accuracy_cases()
    assert len(cases) == len(M.ACCURACY_BIT_FRAMES) * len(M.ACCURACY_SNR) == 93
    assert sorted({bf for bf, _ in cases}) == [bf for bf in M.VALID_BIT_FRAMES if bf <= 1000]
    for bf, x in cases:
        got = M.detect(x)
        assert got["bit_frames"] == bf, (bf, got)
        assert got["score"] < got["runner_up"]


def test_model_rules_short_streams_ties_and_the_runner_up():
    rng = np.random.default_rng(3)
    x = rng.integers(-20000, 20000, 5000).astype(np.int16)
    assert M.detect(x[:4095], [40, 80]) == dict(bit_frames=0, score=-1, runner_up=-1, clock_idx=-1, scores=[-1, -1])
    one = M.detect(x, [40])
    assert one["runner_up"] == -1 and one["scores"] == [one["score"]]
    twice = M.detect(x, [40, 40])
    assert twice["runner_up"] == twice["score"] == one["score"] and twice["bit_frames"] == 40
    zeros = M.detect(np.zeros(4096, np.int16))
    assert zeros["clock_idx"] == 0 and zeros["bit_frames"] == 4 and set(zeros["scores"]) == {32767}


def test_argument_checks_that_need_no_device():
    """(d) the candidate list is checked before anything touches a device."""
    for fn in (lambda c: batch.detect_rates(None, None, None, candidates=c),
               lambda c: modem.detect_baud([np.zeros(5000, np.int16)], candidates=c),
               lambda c: modem.load_batch_auto(["nowhere.wav"], candidates=c)):
        for cands in ([], list(range(4, 4 * 38, 4))):
            with pytest.raises(ValueError, match="candidates"):
                fn(cands)
        for cands, exc in (([40, 44], Exception), ([0], Exception), ([40, -40], Exception), ([2400], IndexError),
                           ([50], Exception)):
            with pytest.raises(exc):
                fn(cands)
    assert batch.check_candidates(None) == batch.VALID_BIT_FRAMES
    assert batch.check_candidates(np.array([160, 40, 40])) == (160, 40, 40)
    assert modem.detect_baud([]) == [] and modem.load_batch_auto([]) == []
    assert afskmodem.detect_baud is modem.detect_baud and afskmodem.load_batch_auto is modem.load_batch_auto
    with pytest.raises(TypeError, match="max_score"):
        modem.load_batch_auto(["nowhere.wav"], max_score="low")
    with pytest.raises(TypeError, match="file names or all"):
        modem._ingest_sources(["a.wav", np.zeros(4, np.int16)])
    host = batch.HostRateResult(np.array([40, 0, 160], np.int32), None, None, None, None, (40, 160))
    assert host.bauds() == [1200, None, 300]
