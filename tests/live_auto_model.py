"""A CPU model of the auto-rate streaming live receiver (``LiveReceiver(n, "auto")``, afsk_live_auto.hip), composed of
what is already pinned down: the oracle's gate over a channel's whole capture, then per burst the detector's model
(tests/detect_model.py) on the burst's first 4096 samples, then a fixed-rate demodulation of the burst at the rate the
detector names -- the streaming model (tests/live_stream_model.py, with ``corrected``) or the oracle's demod_batch.
Also the seeded captures the CPU and the GPU tests of the auto receiver share.  Not a test module."""
from __future__ import annotations

import numpy as np

import afskmodem_amd as afskmodem
from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests import detect_model as D
from tests.live_stream_model import demod_streaming

BLOCK = 2048
FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")
SEED_RATES, SEED_LARGE, SEED_NOISE, SEED_THRESHOLDS = 2, 12, 5, 9     # the seeds of the cases both suites build
LARGE_CHANNELS = 261                        # 65 whole workgroups of four channels and one more
HALF_SCALE = (1.0, 0.5, 1.0, 1.0, 0.5, 1.0)  # the per-channel threshold case: channels 1 and 4 at half scale ...
HALF_PAIRS = ((18000, 14000), (9000, 7000))  # ... with the second pair
RATES = (8, 1000, 20, 160, 40, 96)          # channel c sends RATES[(c + m) % 6] as its message m: fast -> slow -> fast on
                                            # channel 0, slow -> fast -> slow on channel 1


def burst_row(burst, candidates=None, max_score=None, a_end=14000, maxp=256, demod="model") -> dict:
    """One gated burst (a multiple of 2048 samples) as the auto receiver reports it: the demod fields, ``bytes`` (the
    payload row, truncated at ``maxp``), ``bit_frames`` and ``rate_score`` -- and ``corrected`` with demod="model"."""
    burst = np.asarray(burst, np.int16)
    det = D.detect(burst, candidates)
    row = dict(nbytes=0, nbits=0, clock_idx=-1, term_frame=-1, status=_native.ST_TOO_SHORT, bytes=b"",
               bit_frames=int(det["bit_frames"]), rate_score=int(det["score"]))
    if demod == "model":
        row["corrected"] = 0
    if det["bit_frames"] == 0:                                  # fewer than 4096 samples: no rate, no score
        return row
    if max_score is not None and det["score"] > max_score:      # refused: not demodulated, the score still reported
        row.update(status=_native.ST_INVALID_BAUD, bit_frames=0)
        return row
    bf = int(det["bit_frames"])
    if demod == "model":
        r = demod_streaming(burst, bf, a_end, maxp)
        row.update({f: int(r[f]) for f in FIELDS + ("corrected",)})
        row["bytes"] = bytes(r["bytes"])
    else:
        r = O.demod_batch(burst, [0], [burst.size], [bf], a_end, out_stride=max(maxp, 1))
        row.update({f: int(r[f][0]) for f in FIELDS})
        row["bytes"] = r["bytes"][0, : min(row["nbytes"], maxp)].tobytes()
    assert row["clock_idx"] == det["clock_idx"], "the detector's clock index is the demodulator's"
    return row


def expected(cap, candidates=None, max_score=None, a_start=18000, a_end=14000, maxp=256, demod="oracle") -> list:
    """The bursts of one channel's whole capture: the oracle's gate, then ``burst_row`` per burst, with the gate's
    start, len and flags."""
    want, oe = O.gate_stream(cap, a_start, a_end, 4096)
    out = []
    for j, (s, n) in enumerate(want):
        row = dict(start=s, len=n, flags=_native.LIVE_OPEN_END if (oe and j == len(want) - 1) else 0)
        row.update(burst_row(cap[s: s + n], candidates, max_score, a_end, maxp, demod))
        out.append(row)
    return out


# ------------------------------------------------------------------------------------------------- seeded captures


def noisy(rng, x, sigma):
    if not sigma:
        return np.asarray(x, np.int16)
    noise = rng.standard_normal(x.size, dtype=np.float32) * np.float32(sigma)
    return np.clip(np.rint(x + noise), -32768, 32767).astype(np.int16)


def rated_capture(rng, msgs, gap=3 * BLOCK, sigma=2000.0, training=0.2, scale=1.0):
    """``msgs`` = [(bit_frames, payload), ...] with quiet gaps, in noise: every message starts a random number of
    samples into a block (fewer than its clock search covers from 1000 samples per symbol on), as capture_of in
    tests/test_gpu_live_stream.py.  An entry ``("noise", n_blocks)`` is a full-scale white burst of that many blocks (a
    random sign per sample), ``("block", level)`` one block of that constant level on a block boundary."""
    parts, n = [], 0
    for bf, p in msgs:
        if bf == "noise":
            pad, x = (-n) % BLOCK + gap, (rng.integers(0, 2, p * BLOCK) * 2 - 1).astype(np.int16) * 32767
        elif bf == "block":
            pad, x = (-n) % BLOCK + gap, np.full(BLOCK, p, np.int16)
        else:
            lim = BLOCK if 4096 - 2 * bf >= BLOCK else 4096 - 2 * bf - 8
            pad = (-n) % BLOCK + gap + int(rng.integers(0, lim))
            x = afskmodem.Transmitter(48000 // bf, training).wav_samples(p)
            if scale != 1.0:
                x = (x.astype(np.float64) * scale).astype(np.int16)
        parts += [np.zeros(pad, np.int16), x]
        n += pad + x.size
    parts.append(np.zeros(gap + int(rng.integers(0, BLOCK)), np.int16))
    return noisy(rng, np.concatenate(parts), sigma)


def stack(caps, multiple=1):
    """The captures as rows of one zero-padded [n, total] array, total a multiple of ``multiple``."""
    total = -(-max(c.size for c in caps) // multiple) * multiple
    host = np.zeros((len(caps), total), np.int16)
    for i, c in enumerate(caps):
        host[i, : c.size] = c
    return host


def rate_cases(seed: int, n_channels: int = 6, per_channel: int = 3, nbytes: int = 16, scale=None):
    """``(host [n, total], sent)``: channel c carries ``per_channel`` messages of ``nbytes`` random bytes at rates
    rotated through RATES; ``sent[c]`` = [(bit_frames, payload), ...].  ``scale``: a per-channel amplitude factor."""
    rng = np.random.default_rng(seed)
    sent = [[(RATES[(c + m) % len(RATES)], bytes(rng.integers(0, 256, nbytes, dtype=np.uint8)))
             for m in range(per_channel)] for c in range(n_channels)]
    caps = [rated_capture(rng, sent[c], sigma=2000.0 * (scale[c] if scale else 1.0),
                          scale=scale[c] if scale else 1.0) for c in range(n_channels)]
    return stack(caps), sent


def noise_then_message_cases(seed: int, n_channels: int = 6, nbytes: int = 16):
    """``(host, sent)``: every channel carries a full-scale white-noise burst of five blocks, then one message."""
    rng = np.random.default_rng(seed)
    sent = [(RATES[c % len(RATES)], bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))) for c in range(n_channels)]
    caps = [rated_capture(rng, [("noise", 5), sent[c]]) for c in range(n_channels)]
    return stack(caps), sent


def first_windows(cap, a_start=18000, a_end=14000):
    """The first 4096 samples of every gated burst of a capture that has them."""
    want, _ = O.gate_stream(cap, a_start, a_end, 4096)
    return [cap[s: s + 4096] for s, n in want if n >= 4096]


def score_gap(host, sent):
    """(largest score among the real messages, smallest among the noise bursts) of noise_then_message_cases, by the
    detector's model over all 36 candidates."""
    real, noise = [], []
    for c, cap in enumerate(host):
        wins = first_windows(cap)
        assert len(wins) == 2, c
        noise.append(D.detect(wins[0])["score"])
        det = D.detect(wins[1])
        assert det["bit_frames"] == sent[c][0], (c, det)
        real.append(det["score"])
    return max(real), min(noise)
