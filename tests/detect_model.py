"""numpy model of the rate detector (``batch.detect_rates`` / ``afsk_detect_rate_batch``): its definition restated on
the CPU, integer and exact.  Not a test module; tests/test_detect_host.py ties it to the reference and to the oracle,
tests/test_gpu_detect.py compares the device with it field for field.

For the first 4096 raw samples ``x`` of a stream and a candidate ``bf`` (``tc`` = the training cycle of that rate):

    total(i) = sum_j |tc[j] - x[i + j]|            j < 2 bf,  i in [0, 4096 - 2 bf)
    d(i)     = total(i) // (2 bf)                  ci = the first i with minimal d(i)
    n        = (4096 - 2 bf - 1 - ci) // (2 bf) + 1
    score    = (sum_{k < n} total(ci + k 2 bf)) // (n 2 bf)

The detected rate is the candidate of smallest score, the earliest of the list on a tie.  ``totals`` forms the sums
from running sums of the two arrays |32767 - x| and |-32768 - x| (a template sample is one of the two levels);
``totals_direct`` forms them literally and is what the tests hold ``totals`` against."""
import numpy as np

WINDOW = 4096
MAX_STREAM_LEN = (1 << 30) - (1 << 15)
HI, LO = 32767, -32768
# every bit_frames value batch.validate_bit_frames accepts: the divisors of 48000 that are multiples of 4 below 2048
VALID_BIT_FRAMES = [bf for bf in range(4, WINDOW // 2, 4) if 48000 % bf == 0]


def training_cycle(bf: int) -> np.ndarray:
    """mark ++ space of the rate (the reference's getTrainingCycle): two periods of bf / 2, one period of bf."""
    q, h = bf // 4, bf // 2
    return np.array(([HI] * q + [LO] * q) * 2 + [HI] * h + [LO] * h, np.int64)


def totals_direct(x, bf: int) -> np.ndarray:
    x = np.asarray(x[:WINDOW], np.int64)
    tc = training_cycle(bf)
    return np.array([np.abs(tc - x[i: i + 2 * bf]).sum() for i in range(WINDOW - 2 * bf)], np.int64)


def totals(x, bf: int) -> np.ndarray:
    x = np.asarray(x[:WINDOW], np.int64)
    hi = np.concatenate([[0], np.cumsum(np.abs(HI - x))])
    lo = np.concatenate([[0], np.cumsum(np.abs(LO - x))])
    tc = training_cycle(bf)
    edges = [0] + [j for j in range(1, 2 * bf) if tc[j] != tc[j - 1]] + [2 * bf]
    i = np.arange(WINDOW - 2 * bf)
    out = np.zeros(WINDOW - 2 * bf, np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        run = hi if tc[a] == HI else lo
        out += run[i + b] - run[i + a]
    return out


def candidate(x, bf: int):
    """(score, ci, d(ci)) of one candidate."""
    t = totals(x, bf)
    d = t // (2 * bf)
    ci = int(np.argmin(d))                      # (the first minimum)
    n = (WINDOW - 2 * bf - 1 - ci) // (2 * bf) + 1
    s = int(t[ci + 2 * bf * np.arange(n)].sum())
    assert s < 1 << 29
    return s // (n * 2 * bf), ci, int(d[ci])


def detect(x, candidates=None):
    """One stream: dict(bit_frames, score, runner_up, clock_idx, scores).  ``x`` = the whole stream (its length
    decides whether anything is detected)."""
    cands = list(VALID_BIT_FRAMES if candidates is None else candidates)
    if not 0 <= len(x) <= MAX_STREAM_LEN or len(x) < WINDOW:
        return dict(bit_frames=0, score=-1, runner_up=-1, clock_idx=-1, scores=[-1] * len(cands))
    res = [candidate(x, bf) for bf in cands]
    scores = [r[0] for r in res]
    win = min(range(len(cands)), key=lambda k: (scores[k], k))
    others = [s for k, s in enumerate(scores) if k != win]
    return dict(bit_frames=cands[win], score=scores[win], runner_up=min(others) if others else -1,
                clock_idx=res[win][1], scores=scores)


def detect_batch(streams, candidates=None):
    """Arrays [n] (scores [n, K]) for a list of streams."""
    rows = [detect(s, candidates) for s in streams]
    out = {f: np.array([r[f] for r in rows], np.int32) for f in ("bit_frames", "score", "runner_up", "clock_idx")}
    k = len(VALID_BIT_FRAMES if candidates is None else candidates)
    out["scores"] = np.array([r["scores"] for r in rows], np.int32).reshape(len(rows), k)
    return out


# ---------------------------------------------------------------------------------------------- the accuracy list


def add_noise(x, snr_db, rng) -> np.ndarray:
    """Gaussian noise ``snr_db`` below a full-scale square wave, clipped to int16; None = clean."""
    if snr_db is None:
        return np.asarray(x, np.int16)
    sigma = 32767.0 * 10.0 ** (-snr_db / 20.0)
    y = np.asarray(x, np.float64) + rng.normal(0.0, sigma, len(x))
    return np.clip(np.rint(y), LO, HI).astype(np.int16)


ACCURACY_BIT_FRAMES = [bf for bf in VALID_BIT_FRAMES if bf <= 1000]
ACCURACY_SNR = (None, 10.0, 5.0)
ACCURACY_TRAINING = (0.1, 0.2, 0.3, 0.5)


def accuracy_cases(seed: int = 20261018):
    """The seeded list of (true bf, samples): a transmission at every rate with bf <= 1000 behind a silent lead-in
    of 0 ... 2047 samples, training time 0.1 ... 0.5 s, clean / 10 dB / 5 dB -- one case per (rate, noise level),
    the lead and the training time drawn per case.  Cut to what a detector reads plus a little."""
    from afskmodem_amd import Transmitter
    rng = np.random.default_rng(seed)
    cases = []
    for bf in ACCURACY_BIT_FRAMES:
        for snr in ACCURACY_SNR:
            lead = int(rng.integers(0, 2048))
            tt = ACCURACY_TRAINING[int(rng.integers(0, len(ACCURACY_TRAINING)))]
            sig = Transmitter(48000 // bf, tt).frames(b"rate?")
            x = np.concatenate([np.zeros(lead, np.int16), sig])[: WINDOW + 64]
            if len(x) < WINDOW:                                   # (a short burst: silence behind it)
                x = np.concatenate([x, np.zeros(WINDOW - len(x), np.int16)])
            cases.append((bf, add_noise(x, snr, rng)))
    return cases
