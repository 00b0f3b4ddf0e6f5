"""Host side of the ragged push and pull (no GPU): the C-ABI declarations, their exports and their signature table;
the null-handle checks; a pure-Python model of the ragged walk -- tests/test_live_host.py's walk model with a length
and a flush bit per channel -- against the oracle's whole-capture gate, the slot bound and the tap row's capacity;
and the Python wrappers' refusals of a wrong ``lengths`` or mask."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from oracle import afsk_oracle as O
from tests.live_tap_model import TapChannelModel, tap_cap
from tests.test_live_host import BLOCK, Model, capture_from_blocks, closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_ENTRIES = ("afsk_live_push_ragged", "afsk_live_tx_pull_ragged")
SIGNATURES = _native.LIVE_RAGGED_SIGNATURES          # (a build without the ragged entries has nothing to test here)
LENGTHS = (0, 1, 5, 2047, 2048, 2049, 4000, 6144)


def header():
    return open(os.path.join(ROOT, "include", "afsk_amd.h")).read()


def declared_args(hdr, name):
    """The ctypes argument types of an `extern int name(...)` declaration of the header."""
    params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
    out = []
    for p in params.replace("\n", " ").split(","):
        p = p.strip()
        if "*" in p:
            out.append(C.c_void_p)
        else:
            out.append({"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]])
    return out


def test_header_declares_ragged_entries_in_their_own_table():
    hdr = header()
    for name in RAGGED_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_tx_pull(")
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_push_tap(")
    assert set(_native.LIVE_RAGGED_SIGNATURES) == set(RAGGED_ENTRIES)
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_RAGGED_SIGNATURES"]
    assert len(others) >= 9
    for other in others:
        assert not set(RAGGED_ENTRIES) & set(other)
    for name in RAGGED_ENTRIES:
        res, args = _native.LIVE_RAGGED_SIGNATURES[name]
        assert res is C.c_int and args == declared_args(hdr, name), name
    # every argument of the tapped push / the pull, and the device arrays behind chunk_len / flush / n_samples
    push = _native.LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1]
    tap = _native.LIVE_TAP_SIGNATURES["afsk_live_push_tap"][1]
    assert push[:4] + [push[5]] + push[7:] == tap and push[4] is C.c_void_p and push[6] is C.c_void_p
    pull = _native.LIVE_RAGGED_SIGNATURES["afsk_live_tx_pull_ragged"][1]
    assert pull[:4] + pull[5:] == _native.LIVE_TX_SIGNATURES["afsk_live_tx_pull"][1]
    assert declared_args(hdr, "afsk_live_push_tap") == tap
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert "one captured graph" in hdr.lower()


def test_library_exports_ragged_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in RAGGED_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2        # binds every table
    assert _native.lib().afsk_live_push_ragged.argtypes == _native.LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1]


def test_entries_refuse_null_handles_without_a_device():
    lib = _native.lib()
    null_push = [None, None, 0, 0, None, 0, None] + [None] * 5 + [0] + [None] * 7 + [0] + [None] * 6
    assert len(null_push) == len(_native.LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1])
    assert lib.afsk_live_push_ragged(*null_push) == _native.E_INVALID_ARG
    assert "null live receiver" in _native.last_error()
    pending = np.zeros(4, np.int32)
    assert lib.afsk_live_tx_pull_ragged(None, None, 0, 0, None, pending.ctypes.data, None) == _native.E_INVALID_ARG
    assert "null live transmitter" in _native.last_error()


# ----------------------------------------------------------------------------------------- the ragged walk, modelled

class RaggedModel:
    """live_gate_walk's RAGGED form over n channels: channel c walks clamp(lengths[c], 0, T) samples with
    tests/test_live_host.py's Model and flushes when ``flush`` or ``mask[c]``."""

    def __init__(self, amps):
        self.chan = [Model(lambda b, a=a: int(a[b])) for a in amps]

    def push(self, T, lengths=None, flush=False, mask=None):
        out = []
        for c, m in enumerate(self.chan):
            ln = T if lengths is None else min(max(int(lengths[c]), 0), T)
            before = (m.pos, m.mode, m.rec_start, m.rec_len)
            fl = bool(flush) or (mask is not None and bool(mask[c]))
            got = m.push(ln, flush=fl)
            if ln == 0 and not fl:                                  # the state is kept exactly, nothing is reported
                assert got == [] and before == (m.pos, m.mode, m.rec_start, m.rec_len)
            out.append(got)
        return out


def schedule(rng, totals, T, lengths=LENGTHS):
    """Per push (lengths [n], mask [n]): every channel's own lengths summing to its total; a channel that has
    finished pushes 0 and gets its flush bit once -- with its last samples or in a later push of length 0."""
    n = len(totals)
    left = list(totals)
    flushed = [False] * n
    wait = [int(rng.integers(0, 3)) for _ in range(n)]              # empty pushes before the flush bit
    out = []
    while not all(flushed):
        lens, mask = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        for c in range(n):
            if flushed[c]:
                continue
            t = min(int(rng.choice(lengths)), left[c], T)
            if left[c] == 0:
                t = 0
            left[c] -= t
            lens[c] = t
            if left[c] == 0:
                if wait[c] == 0:
                    mask[c], flushed[c] = 1, True
                else:
                    wait[c] -= 1
        out.append((lens, mask))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_any_ragged_schedule_followed_by_a_flush_gives_the_oracles_bursts(seed):
    rng = np.random.default_rng(seed)
    n, T = 8, 6144
    slots, _ = closed_form(1, 96000, T)
    caps, amps = [], []
    for c in range(n):
        nb = int(rng.integers(0, 40))
        a = rng.choice([0, 5000, 14000, 16000, 18000, 18001, 25000], nb) if c % 3 else \
            np.resize(np.array([0, 30000, 30000]), nb)
        cap = capture_from_blocks(rng, a, int(rng.integers(0, BLOCK)))
        caps.append(cap)
        amps.append([O.get_amplitude(cap[BLOCK * b: BLOCK * b + BLOCK]) for b in range(len(cap) // BLOCK)])
    model = RaggedModel(amps)
    got = [[] for _ in range(n)]
    sched = schedule(rng, [len(c) for c in caps], T)
    assert any(len({int(x) for x in lens if x > 0}) > 1 for lens, _ in sched)          # ragged indeed
    for lens, mask in sched:
        for c, bursts in enumerate(model.push(T, lens, mask=mask)):
            assert len(bursts) <= slots                                             # 1 + k_blocks / 3
            got[c] += bursts
    for c in range(n):
        want, oe = O.gate_stream(caps[c], 18000, 14000, 64)
        assert [(s, ln) for s, ln, _ in got[c]] == want, c
        assert [f for _, _, f in got[c]] == [0] * (len(want) - oe) + [_native.LIVE_OPEN_END] * oe, c
        assert model.chan[c].pos == 0 and model.chan[c].mode == 0                     # flushed: a new stream


def test_lengths_are_clamped_and_none_means_every_column():
    amps = [[0, 30000, 30000, 0, 0, 0] * 2] * 3
    a, b = RaggedModel(amps), RaggedModel(amps)
    for _ in range(2):
        got = a.push(6144, [-5, 6144 + 100, 6144])
        want = b.push(6144, [0, 6144, 6144])
        assert got == want
    assert [m.pos for m in a.chan] == [0, 12288, 12288]
    assert a.push(6144) == b.push(6144, [6144] * 3)
    assert a.push(0, flush=True) == b.push(0, mask=[1, 1, 1])


@pytest.mark.parametrize("mc", [2047, 2049, 6144, 8192])
def test_the_slot_bound_holds_for_ragged_pushes(mc):
    """len_c <= chunk_len <= max_chunk_len: a ragged push walks at most the blocks a plain push of max_chunk_len
    walks, so 1 + k_blocks / 3 slots are enough -- also with bursts that close every third block."""
    slots, _ = closed_form(1, 96000, mc)
    rng = np.random.default_rng(mc)
    most = 0
    for trial in range(100):
        n = 4
        nbs = rng.integers(0, 60, n)
        amps = [np.resize(np.array([30000, 30000, 0]), nb) if (trial + c) % 2 else
                rng.choice([0, 16000, 20000, 30000], nb, p=[0.35, 0.1, 0.25, 0.3]) for c, nb in enumerate(nbs)]
        model = RaggedModel(amps)
        totals = [int(nb) * BLOCK + int(rng.integers(0, BLOCK)) for nb in nbs]
        for lens, mask in schedule(rng, totals, mc, lengths=(0, 1, 2047, 2049, mc, mc, mc)):
            for bursts in model.push(mc, lens, mask=mask):
                most = max(most, len(bursts))
    assert 0 < most <= slots


@pytest.mark.parametrize("bf", [8, 40])
def test_tap_cap_bounds_a_ragged_push(bf):
    """AFSK_LIVE_TAP_CAP(max_chunk_len, bf) bounds what a channel commits in one push of ANY length up to
    max_chunk_len: continuous data, every push's length drawn from the ragged set."""
    rng = np.random.default_rng(bf)
    T = 6144
    cap = tap_cap(T, bf)
    data = bytes(rng.integers(0, 256, 40 * BLOCK // (14 * bf), dtype=np.uint8))
    msg = O.get_frames(data, 48000 // bf, 2.5 * bf / 48000).astype(np.int16)
    stream = np.concatenate([np.zeros(BLOCK + 77, np.int16), msg, np.zeros(3 * BLOCK, np.int16)])
    worst = 0
    for trial in range(4):
        ch = TapChannelModel(bf)
        p = 0
        while p < stream.size:
            t = min(int(rng.choice(LENGTHS)), stream.size - p)
            r = ch.push(stream[p:p + t])
            worst = max(worst, len(r["tap"]))
            if t == 0:
                assert r["tap"] == b"" and r["bursts"] == []
            p += t
    assert 0 < worst <= cap, (worst, cap)


# -------------------------------------------------------------------------------------------- the Python wrappers

def test_lengths_and_mask_argument_checks():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    for bad in ([1, 2, 3], np.zeros((4, 1), np.int32), np.zeros(5, np.int64), 7):
        with pytest.raises(ValueError, match="n_channels=4"):
            live._device_lengths(bad, 4, dev, "receiver")                                  # a wrong shape
    for bad in ([1.0, 2.0, 3.0, 4.0], np.zeros(4, np.float32), np.zeros(4, bool)):
        with pytest.raises(TypeError, match="integer"):
            live._device_lengths(bad, 4, dev, "receiver")                                  # a wrong dtype
    for dt in (torch.int64, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="int32"):
            live._device_lengths(torch.zeros(4, dtype=dt), 4, dev, "receiver")
    with pytest.raises(ValueError, match="lengths is on cpu, the receiver on cuda:0"):
        live._device_lengths(torch.zeros(4, dtype=torch.int32), 4, dev, "receiver")        # another device
    with pytest.raises(ValueError, match="the transmitter on cuda:0"):
        live._device_lengths(torch.zeros(4, dtype=torch.int32), 4, dev, "transmitter")
    for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.float16), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(TypeError, match="flush mask"):
            live._flush_mask(bad, 4, dev)                                                  # a float tensor as the mask
    with pytest.raises(TypeError, match="flush mask"):
        live._flush_mask(np.zeros(4, np.float64), 4, dev)
    # the keywords exist on the public methods
    import inspect
    assert "lengths" in inspect.signature(live.LiveReceiver.push).parameters
    assert {"mask", "lengths"} <= set(inspect.signature(live.LiveReceiver.flush).parameters)
    assert "lengths" in inspect.signature(live.LiveTransmitter.pull).parameters
