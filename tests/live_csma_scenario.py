"""The two-stations-on-one-channel scenario of the half-duplex tests, on the models alone (tests/live_csma_model.py):
PAIRS media, each shared by channel c of station A, channel c of station B and a third sender.  The third sender's
burst holds both stations off while each gets a message of its own to send; when the burst ends both are released by
the same block.  tests/test_live_csma_host.py asserts what the committed seeds give; tests/test_gpu_live_csma.py drives
two real stations through the same ticks and compares every one with ``run``'s record.  Not a test module."""
from types import SimpleNamespace

import numpy as np

import afskmodem_amd as afskmodem
from tests import live_csma_model as M

PAIRS, T, TICKS = 8, 2048, 60
DEPTH, MAXP = 4, 16
TR = afskmodem.Transmitter(1200, 0.05)                       # both stations: 6 bytes are 5920 tone samples
THIRD = afskmodem.Transmitter(1200, 0.1).wav_samples(b"thirdone")   # 9440 tone samples + the silent tail
THIRD_AT = T + 100                                           # inside the second block
SUBMIT_TICK = 3                                              # both stations get their messages while they are held
RELEASE_TICK = 6                                             # the first tick whose block is quiet again
HOLDOFF = 4800                                               # past the block every gate discards after a burst
SEED_A, SEED_B = 3, 45                                       # chosen on the model: see test_live_csma_host.py
_rng = np.random.default_rng(99)
PAY = [[bytes(_rng.integers(0, 256, 6, dtype=np.uint8)) for _ in range(PAIRS)] for _ in range(2)]


def third_samples() -> np.ndarray:
    x = np.zeros((PAIRS, TICKS * T), np.int16)
    x[:, THIRD_AT: THIRD_AT + THIRD.size] = THIRD
    return x


def CsmaScenario(persist: int, slot: int, seeds, mute: bool = True, holdoff: int = HOLDOFF) -> M.SharedChannel:
    stations = [M.CsmaTxModel(PAIRS, 40, TR.ts_cycles, DEPTH, MAXP, wav=TR.wav_samples) for _ in range(2)]
    return M.SharedChannel(stations, third_samples(), T, holdoff, persist, slot, seeds, mute=mute)


def start_when_released() -> int:
    """Where a message begins that waited through the third burst with no slots drawn."""
    return RELEASE_TICK * T + HOLDOFF


def run(ch: M.SharedChannel, ticks: int = TICKS):
    """Tick until both stations have sent everything and the medium has been quiet for four ticks (or ``ticks``).
    The record: per tick ``medium`` [PAIRS, T], ``heard`` / ``busy`` / ``samples`` / ``pending`` / ``deferred`` /
    ``on_air`` per station; ``starts[s][c]``: the sample at which station s's channel c first had tones on air."""
    r = SimpleNamespace(medium=[], heard=[], busy=[], samples=[], pending=[], deferred=[], on_air=[],
                        starts=[[None] * PAIRS for _ in range(2)], done=False)
    quiet = 0
    for t in range(ticks):
        if t == SUBMIT_TICK:
            for s, st in enumerate(ch.st):
                status, _, _ = st.submit(list(range(PAIRS)), PAY[s])
                assert not status.any()
        chunk, heard, busy, pulls = ch.tick()
        r.medium.append(chunk)
        r.heard.append(heard)
        r.busy.append(busy)
        for name, i in (("samples", 0), ("pending", 1), ("deferred", 2), ("on_air", 3)):
            getattr(r, name).append([np.array(p[i], copy=True) for p in pulls])
        for s in range(2):
            for c in range(PAIRS):
                lo, hi = pulls[s][3][c]
                if hi > lo and r.starts[s][c] is None:
                    r.starts[s][c] = t * T + int(lo)
        r.done = t > SUBMIT_TICK and not any(st.pending().any() for st in ch.st)
        quiet = quiet + 1 if r.done and not chunk.any() else 0
        if quiet >= 4:
            break
    return r
