"""CPU suite of the auto-rate streaming live receiver (``LiveReceiver(n, "auto")``): the model the GPU tests compare
the device with (tests/live_auto_model.py) against the fixed-rate streaming model, the condition the GPU tests rest on
-- the detector's model alone names the true rate of every message of every seeded capture they use -- the tie rule, the
``max_score`` gap, the constructor's argument errors (raised before any device is looked for) and the C declarations."""
import os
import re

import numpy as np
import pytest

from afskmodem_amd import _native, batch
from afskmodem_amd.live import LiveEvents, LiveReceiver, LiveResult
from oracle import afsk_oracle as O
from tests import detect_model as D
from tests import live_auto_model as M
from tests.live_stream_model import demod_streaming

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 2048


@pytest.mark.parametrize("r", [8, 40, 160, 1000])
def test_one_candidate_is_the_fixed_rate_streaming_model(r):
    """E1 on the model: with candidates=[r] every burst is what the fixed-rate streaming model makes of it, and the
    reported rate is r for every burst that reached 4096 samples."""
    rng = np.random.default_rng(r)
    cap = M.rated_capture(rng, [(r, b"0123456789abcdef"), ("block", 30000), (r, b"second message!!")])
    cap = cap[: cap.size - cap.size % BLOCK - BLOCK]
    want, oe = O.gate_stream(cap, 18000, 14000, 4096)
    rows = M.expected(cap, [r], demod="model")
    assert len(rows) == len(want) == 3
    for (s, n), row in zip(want, rows):
        fixed = demod_streaming(cap[s: s + n], r)
        for f in M.FIELDS + ("corrected", "bytes"):
            assert row[f] == fixed[f], (f, row[f], fixed[f])
        assert row["bit_frames"] == r and row["rate_score"] == D.candidate(cap[s: s + 4096], r)[0]
    assert [row["bytes"] for row in rows][::2] == [b"0123456789abcdef", b"second message!!"]
    # fewer than 4096 samples: no rate, no score, TOO_SHORT
    short = M.burst_row(cap[want[0][0]: want[0][0] + BLOCK], [r])
    assert (short["status"], short["bit_frames"], short["rate_score"]) == (_native.ST_TOO_SHORT, 0, -1)


def check_rates(host, sent, scale=None):
    for c, cap in enumerate(host):
        pair = M.HALF_PAIRS[scale[c] != 1.0] if scale else M.HALF_PAIRS[0]
        rows = M.expected(cap, None, None, pair[0], pair[1])
        assert [(row["bit_frames"], row["bytes"]) for row in rows] == list(sent[c]), c


def test_the_model_names_the_true_rate_in_every_seeded_case_of_the_gpu_tests():
    check_rates(*M.rate_cases(M.SEED_RATES))
    check_rates(*M.rate_cases(M.SEED_THRESHOLDS, scale=M.HALF_SCALE), scale=M.HALF_SCALE)


def test_the_model_names_the_true_rate_of_every_channel_of_the_large_case():
    check_rates(*M.rate_cases(M.SEED_LARGE, M.LARGE_CHANNELS, 1))


def test_noise_bursts_score_above_every_real_message():
    host, sent = M.noise_then_message_cases(M.SEED_NOISE)
    real, noise = M.score_gap(host, sent)
    assert 0 <= real < noise - 1, (real, noise)
    limit = (real + noise) // 2
    for c, cap in enumerate(host):
        rows = M.expected(cap, None, limit)
        assert [row["status"] for row in rows] == [_native.ST_INVALID_BAUD, _native.ST_OK], c
        refused = rows[0]
        assert (refused["bit_frames"], refused["nbytes"], refused["nbits"], refused["clock_idx"], refused["term_frame"],
                refused["bytes"]) == (0, 0, 0, -1, -1, b"")
        assert refused["rate_score"] > limit >= rows[1]["rate_score"]
        assert (rows[1]["bit_frames"], rows[1]["bytes"]) == sent[c]


def test_every_candidate_ties_on_a_constant_full_scale_burst_and_the_earliest_wins():
    x = np.full(5 * BLOCK, 32767, np.int16)
    assert set(D.detect(x)["scores"]) == {32767}
    for cands, want in (([160, 40], 160), ([40, 160], 40), ([40, 40, 160], 40)):
        row = M.burst_row(x, cands)
        assert (row["bit_frames"], row["rate_score"], row["clock_idx"]) == (want, 32767, 0), cands


def test_argument_errors_come_before_the_device_check():
    with pytest.raises(ValueError, match="streaming receiver"):
        LiveReceiver(4, "auto")                                            # (the default is a stored receiver)
    with pytest.raises(ValueError, match="streaming receiver"):
        LiveReceiver(4, "auto", max_burst_len=48000)
    for bad in ([], list(batch.VALID_BIT_FRAMES) + [40]):                  # 1 ... 36 candidates
        with pytest.raises(ValueError, match="candidates"):
            LiveReceiver(4, "auto", max_burst_len=None, candidates=bad)
    # a candidate no Receiver has: the reference's own errors, as LiveReceiver(4, 42) raises them
    for bad, kind in (([40, 42], Exception), ([0], Exception), ([-40], Exception), ([40, 4000], IndexError),
                      ([40, 50], Exception)):
        with pytest.raises(kind) as e:
            LiveReceiver(4, "auto", max_burst_len=None, candidates=bad)
        assert type(e.value) is kind and "device" not in str(e.value).lower(), bad
    for bad in (-1, 1.5, 2 ** 31):
        with pytest.raises(ValueError, match="max_score"):
            LiveReceiver(4, "auto", max_burst_len=None, max_score=bad)
    with pytest.raises(ValueError, match='"auto"'):
        LiveReceiver(4, 40, max_burst_len=None, candidates=[40])
    with pytest.raises(ValueError, match='"auto"'):
        LiveReceiver(4, 40, max_burst_len=None, max_score=100)
    with pytest.raises(ValueError):
        LiveReceiver(4, "fast", max_burst_len=None)


def test_results_of_other_receivers_have_no_rates():
    z = np.zeros((2, 1), np.int32)
    res = LiveResult(np.zeros(2, np.int32), z.astype(np.int64), z, z, None)
    assert res.bit_frames is None and res.rate_score is None
    with pytest.raises(ValueError, match="auto receiver"):
        res.rated_bursts()
    ev = LiveEvents(np.zeros(32 + 48, np.uint8), 1, 0, result=res)
    with pytest.raises(ValueError, match="auto receiver"):
        ev.bit_frames()
    with pytest.raises(ValueError, match="auto receiver"):
        LiveEvents(np.zeros(32 + 48, np.uint8), 1, 0).bit_frames()


def ctypes_of(hdr, name):
    """The ctypes argument types of an `extern int name(...)` declaration of the header."""
    import ctypes as C
    params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
    out = []
    for p in re.sub(r"/\*.*?\*/", "", params, flags=re.S).split(","):
        p = " ".join(p.split())
        if "*" in p:
            host_i32 = p.startswith("const int32_t *") and p.endswith("_host")
            out.append(C.POINTER(C.c_void_p) if "**" in p else C.POINTER(C.c_int32) if host_i32 else C.c_void_p)
        else:
            out.append({"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]])
    return out


def test_the_bindings_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    for name, (_, args) in _native.LIVE_AUTO_SIGNATURES.items():
        assert ctypes_of(hdr, name) == args, name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_detect_rate_batch(")
    ragged = _native.LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1]
    assert len(_native.LIVE_AUTO_SIGNATURES["afsk_live_push_auto"][1]) == len(ragged) + 2
    assert _native.DETECT_MAX_CANDIDATES == len(batch.VALID_BIT_FRAMES) == 36
