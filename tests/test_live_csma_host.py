"""Host side of the half-duplex additions of the live side (no GPU): the C-ABI declarations of afsk_live_tx_pull_csma,
afsk_live_push_muted and afsk_live_push_auto_muted, their signature table and the library's exports; the csma model
(tests/live_csma_model.py) against hand-worked cases -- the hash, persist = 255 is the hold model, the statistics of the
draw, the cap, the int32 bound, ``on_air`` -- the mute clamping; the two-station scenario the GPU test replays, for its
committed seeds; and the refusals of ``LiveTransmitter.pull(persist=)`` / ``LiveReceiver.push(mute=)`` that need no
device."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from tests import live_csma_model as M
from tests import live_csma_scenario as S
from tests import live_tx_hold_model as H
from tests.test_live_ragged_host import header
from oracle import afsk_oracle as O   # the scenario's monitor: the reference's gate and demodulator on the medium

ENTRIES = ("afsk_live_tx_pull_csma", "afsk_live_push_muted", "afsk_live_push_auto_muted")
TR = afskmodem.Transmitter(1200, 0.0)            # a message of p bytes: 40 * (4 + 14 p) + 4800 samples


def declared_args(hdr, name):
    """The ctypes argument types of an `extern int name(...)` declaration of the header (with uint32_t, which the
    helper of tests/test_live_ragged_host.py has no need for)."""
    params = re.search(r"^extern int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
    return [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in params.replace("\n", " ").split(",")]


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_CSMA_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_CSMA_SIGNATURES[name]
        assert res is C.c_int and args == declared_args(hdr, name), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_tx_pull_hold(")
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_CSMA_SIGNATURES"]
    assert len(others) >= 17 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    # the hold pull's arguments with persist, slot and seed behind holdoff and out_on_air behind out_deferred
    hold = _native.LIVE_TX_HOLD_SIGNATURES["afsk_live_tx_pull_hold"][1]
    csma = _native.LIVE_CSMA_SIGNATURES["afsk_live_tx_pull_csma"][1]
    assert csma[:7] + csma[10:12] + [csma[13]] == hold
    assert csma[7:10] == [C.c_int32, C.c_int32, C.c_uint32] and csma[12] is C.c_void_p
    # the ragged / auto push's arguments with d_mute behind the flush mask
    for muted, base in (("afsk_live_push_muted", _native.LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1]),
                        ("afsk_live_push_auto_muted", _native.LIVE_AUTO_SIGNATURES["afsk_live_push_auto"][1])):
        args = _native.LIVE_CSMA_SIGNATURES[muted][1]
        assert args[:7] + args[8:] == base and args[7] is C.c_void_p
    for word in ("persist", "0x7feb352d", "0x846ca68b", "0x9e3779b9", "out_on_air", "d_mute", "KISS"):
        assert word in hdr


def test_library_exports_and_binds_the_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_CSMA_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


def test_null_handles_are_refused_before_a_device_is_needed():
    lib = _native.lib()
    assert lib.afsk_live_tx_pull_csma(None, None, 0, 0, None, None, 0, 255, 0, 0, None, None, None,
                                      None) == _native.E_INVALID_ARG
    assert "null live transmitter" in _native.last_error()
    for name in ENTRIES[1:]:
        args = [0 if t in (C.c_int32, C.c_int64) else None for t in _native.LIVE_CSMA_SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == _native.E_INVALID_ARG
        assert "null live receiver" in _native.last_error()


# ------------------------------------------------------------------------------------------------------ the draw

def test_hash32_against_hand_computed_values():
    # 1: x ^= x >> 16 -> 1; * 0x7feb352d -> 0x7feb352d; ^= >> 15 -> 0x7feb352d ^ 0xffd6 = 0x7febcafb; * 0x846ca68b
    # mod 2^32 -> 0x6889f849; ^= >> 16 -> 0x6889f849 ^ 0x6889 = 0x688990c0.  The other two were worked the same way,
    # with plain 32-bit integer arithmetic.
    assert M.hash32(0) == 0
    assert M.hash32(1) == 0x688990C0
    assert M.hash32(0x9E3779B9) == 0x01FCE552
    assert M.hash32(0xFFFFFFFF) == 0x6768824A
    assert M.hash32(np.array([1, 0xFFFFFFFF])).tolist() == [0x688990C0, 0x6768824A]
    assert M.hash32(2 ** 32 + 1) == M.hash32(1)                   # uint32: the upper bits do not exist


def test_the_share_of_no_wait_and_the_mean_wait_at_persist_63():
    c, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    g = M.slots_drawn_many(0, c, k, 63)
    assert g.shape == (256, 256)
    sigma = math.sqrt(0.25 * 0.75 / 65536)
    assert abs(sigma * 5 - 0.0085) < 0.0001
    share = float((g == 0).mean())
    assert abs(share - 0.25) <= 5 * sigma, share
    # G is geometric with p = 1/4: mean (1 - p) / p = 3, variance (1 - p) / p^2 = 12 (the cap at 255 is out of reach)
    mean = float(g.mean())
    assert abs(mean - 3.0) <= 5 * math.sqrt(12 / 65536), mean
    assert g.max() < 255
    for cc, kk in ((0, 0), (3, 7), (255, 255), (17, 200)):         # the array form is the scalar one
        assert g[cc, kk] == M.slots_drawn(0, cc, kk, 63)
    # every channel and every draw has its own sequence; the seed changes all of them
    assert len({tuple(r) for r in g.tolist()}) == 256 and len({tuple(r) for r in g.T.tolist()}) == 256
    assert (M.slots_drawn_many(1, c, k, 63) != g).mean() > 0.5


def test_persist_255_never_waits_and_255_slots_are_reached_only_by_the_cap():
    c, k = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    assert not M.slots_drawn_many(9, c, k, 255).any()
    assert M.slots_drawn(9, 5, 5, 255, h=lambda x: 0xFFFFFFFF) == 0            # 255 <= 255: the first slot
    assert M.slots_drawn(9, 5, 5, 254, h=lambda x: 0xFFFFFFFF) == 255          # no slot is ever taken: the cap
    base = int(M.draw_base(9, 5, 5))
    assert M.slots_drawn(9, 5, 5, 0, h=lambda x: 0 if x == base ^ 254 else 0xFF) == 254   # the last slot that counts
    assert M.slots_drawn(9, 5, 5, 0, h=lambda x: 0 if x == base ^ 255 else 0xFF) == 255   # j = 255 is not drawn
    g = M.slots_drawn_many(3, c, k, 0)                                          # p = 1 / 256: (255/256)^255 = 37 % cap
    assert 0.25 < float((g == 255).mean()) < 0.5 and g.min() >= 0


def test_the_wait_fits_int32_at_the_argument_bounds():
    worst = _native.MAX_STREAM_LEN + M.SLOT_MAX * 255
    assert worst < 2 ** 31
    m = M.CsmaTxModel(1, 40, 0, 4, 64, wav=TR.wav_samples)
    m.pull_csma(16, hold=[1], holdoff=_native.MAX_STREAM_LEN, persist=254, slot=M.SLOT_MAX, seed=1)
    assert m.wait[0] == _native.MAX_STREAM_LEN + M.SLOT_MAX * M.slots_drawn(1, 0, 0, 254) < 2 ** 31
    assert m.draws == [1]


# ------------------------------------------------------------------------------------------------ the csma model

def twins(n=1, depth=4):
    return (M.CsmaTxModel(n, 40, 0, depth, 64, wav=TR.wav_samples),
            H.HoldTxModel(n, 40, 0, depth, 64, wav=TR.wav_samples))


def test_persist_255_is_the_hold_model_on_its_hand_worked_cases():
    # the script of tests/test_live_tx_hold_host.py::test_hand_worked_hold_and_holdoff, on both models
    a, b = twins()
    for m in (a, b):
        m.submit([0, 0], [b"", b"a"])
    script = [dict(T=1000, hold=[1], holdoff=300), dict(T=1000, hold=[0], holdoff=300),
              dict(T=5000, hold=[1], holdoff=10000), dict(T=4000, hold=None, holdoff=0), dict(T=4000),
              dict(T=4000, lens=[0], hold=[1], holdoff=77, fill=9), dict(T=9000, hold=[0], holdoff=5)]
    want_deferred = [1000, 300, 7000 - 6260, 10000, 0, 0]
    for k, kw in enumerate(script):
        T = kw.pop("T")
        got = a.pull_csma(T, persist=255, slot=4800, seed=77, **kw)
        want = b.pull_hold(T, **kw)
        for g, w in zip(got[:3], want):
            assert (g == w).all(), k
        if k < len(want_deferred):
            assert got[2].tolist() == [want_deferred[k]]
        assert a.wait == b.wait and a.pos == b.pos and a.end == b.end and list(a.queue[0]) == list(b.queue[0]), k
    assert a.draws == [3]                                         # one draw per held pull, whatever it drew
    a.reset([True])
    assert a.draws == [0] and a.wait == [0]
    # a seeded script of submits and pulls
    rng = np.random.default_rng(8)
    a, b = twins(3, 3)
    for _ in range(60):
        k = int(rng.integers(0, 4))
        chans = sorted(rng.integers(0, 3, k).tolist())
        pays = [bytes(rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8)) for _ in range(k)]
        for x, y in zip(a.submit(chans, pays), b.submit(chans, pays)):
            assert (x == y).all()
        T = int(rng.choice([1, 700, 2048, 4099, 9000]))
        hold = rng.integers(0, 2, 3).tolist()
        holdoff = int(rng.choice([0, 1, 4097]))
        got, want = a.pull_csma(T, hold=hold, holdoff=holdoff, persist=255, slot=99), b.pull_hold(T, hold=hold,
                                                                                                 holdoff=holdoff)
        assert all((g == w).all() for g, w in zip(got[:3], want)) and a.wait == b.wait


def test_a_held_channel_waits_its_holdoff_and_the_slots_it_drew():
    m = M.CsmaTxModel(2, 40, 0, 4, 64, wav=TR.wav_samples, channel_ids=[5, 9])
    m.submit([0, 1], [b"ab", b"ab"])
    seed, persist, slot = 11, 63, 1000
    g = [[M.slots_drawn(seed, c, k, persist) for k in range(3)] for c in (5, 9)]
    assert any(x for r in g for x in r) and g[0] != g[1]
    kw = dict(holdoff=300, persist=persist, slot=slot, seed=seed)
    m.pull_csma(2048, hold=[1, 1], **kw)
    assert m.wait == [300 + slot * g[0][0], 300 + slot * g[1][0]] and m.draws == [1, 1]
    m.pull_csma(2048, hold=[1, 0], **kw)                           # channel 0 draws again, channel 1 counts down
    assert m.wait[0] == 300 + slot * g[0][1] and m.draws == [2, 1]
    assert m.wait[1] == max(0, 300 + slot * g[1][0] - 2048)
    assert list(m.queue[1])[0][0] == 2048 + 300 + slot * g[1][0]   # released: it begins where its wait ends
    # the other pulls neither read nor write k
    m.pull_hold(100, hold=[1, 1], holdoff=7)
    m.pull(100)
    assert m.draws == [2, 1] and m.wait == [7, 7]
    m.pull_csma(0, hold=[1, 0], **kw)                              # L = 0, held: draws, shifts nothing
    assert m.draws == [3, 1] and m.wait[0] == 300 + slot * g[0][2]


def test_on_air():
    n = TR.wav_samples(b"ab").size                                 # 40 * 32 + 4800
    tones = n - 4800
    assert tones == 1280
    m = M.CsmaTxModel(1, 40, 0, 4, 64, wav=TR.wav_samples)
    air = lambda *a, **kw: m.pull_csma(*a, **kw)[3].tolist()       # noqa: E731
    assert air(500) == [[0, 0]]                                    # an empty queue
    m.submit([0], [b"ab"])                                         # starts at 500
    m.pull_csma(100, hold=[1], holdoff=300)                        # held: start 600, then the wait of 300: 900
    assert air(1000) == [[300, 1000]]                              # a message that starts mid-pull (pos 600)
    assert air(0) == [[0, 0]]                                      # L = 0
    assert air(1000, lens=[0]) == [[0, 0]]
    assert air(1000) == [[0, 900 + tones - 1600]]                  # ... and ends mid-pull (pos 1600, tones end 2180)
    assert air(1000) == [[0, 0]] and m.pending().tolist() == [1]   # only its silent tail in the pull
    # two messages in one pull: the hull, over the first one's silent tail
    m = M.CsmaTxModel(1, 40, 0, 4, 64, wav=TR.wav_samples)
    m.submit([0, 0], [b"ab", b"ab"])
    m.pull_csma(1000)
    out, _, _, oa = m.pull_csma(8000)                              # pos 1000: tones to 1280, then from 6080 to 7360
    assert oa.tolist() == [[0, 7360 - 1000]] and not out[0, 280: 5080].any() and out[0, 5080] != 0
    # a ragged pull cuts the hull at its length; a held one reports what plays on, not what it moved away
    m = M.CsmaTxModel(2, 40, 0, 4, 64, wav=TR.wav_samples)
    m.submit([0, 1], [b"ab", b"ab"])
    assert m.pull_csma(1000, lens=[700, 1000], hold=[0, 1])[3].tolist() == [[0, 700], [0, 0]]
    m.submit([0], [b"ab"])
    assert m.pull_csma(1000, hold=[1, 0])[3].tolist() == [[0, 580], [0, 1000]]


# ------------------------------------------------------------------------------------------------------- mute

def test_mute_ranges_are_clamped():
    T = 100
    mute = [(10, 20), (20, 10), (-5, 7), (-9, -2), (90, 300), (150, 200), (0, 100), (0, 0), (30, 60), (30, 60)]
    lens = [100, 100, 100, 100, 100, 100, 100, 100, 40, 0]
    want = [(10, 20), (20, 20), (0, 7), (0, 0), (90, 100), (100, 100), (0, 100), (0, 0), (30, 40), (0, 0)]
    assert M.mute_ranges(mute, lens, T).tolist() == [list(w) for w in want]
    assert M.mute_ranges(mute, None, T).tolist()[8:] == [[30, 60], [30, 60]]
    assert M.mute_ranges([(5, 9)], [-3], T).tolist() == [[0, 0]] and M.mute_ranges([(5, 9)], [500], T).tolist() == [[5, 9]]
    chunk = np.arange(1, 1 + 10 * T, dtype=np.int16).reshape(10, T)
    out = M.muted(chunk, mute, lens)
    for c, (lo, hi) in enumerate(want):
        assert not out[c, lo:hi].any() and (out[c, :lo] == chunk[c, :lo]).all() and (out[c, hi:] == chunk[c, hi:]).all()
    assert chunk[0, 10] != 0                                       # a copy
    # what the gate hears: a muted loud block is silence
    loud = np.full((1, 3 * H.BLOCK), 20000, np.int16)
    assert H.busy_after(loud[0], [H.BLOCK] * 3) == [0, 1, 1]
    assert H.busy_after(M.muted(loud, [(H.BLOCK, 3 * H.BLOCK)])[0], [H.BLOCK] * 3) == [0, 0, 0]


# --------------------------------------------------------------------------------------------------- the scenario

def monitor(run):
    """What a listener on every medium decodes: the reference's gate over the whole medium, its demodulator on every
    burst."""
    medium = np.concatenate(run.medium, axis=1)
    return [{O.load_frames(medium[c, s: s + n], 1200) for s, n in O.gate_stream(medium[c])[0]} for c in range(S.PAIRS)]


def test_equal_waits_collide_and_drawn_waits_take_turns_for_the_committed_seeds():
    tones = S.TR.wav_samples(S.PAY[0][0]).size - 4800
    # persist = 255: both stations of every pair key up on the same sample, right where the third burst released them
    run = S.run(S.CsmaScenario(255, 0, (S.SEED_A, S.SEED_B)))
    assert run.done and run.starts[0] == run.starts[1] == [S.start_when_released()] * S.PAIRS
    assert not any(d.any() for t, both in enumerate(run.deferred) if t > S.RELEASE_TICK for d in both)   # nobody defers
    for c, heard in enumerate(monitor(run)):
        assert b"thirdone" in heard and S.PAY[0][c] not in heard and S.PAY[1][c] not in heard, c   # neither decodes
    # persist = 63, a slot of 4800 and different seeds: one starts first, the other hears it and defers
    run = S.run(S.CsmaScenario(63, 4800, (S.SEED_A, S.SEED_B)))
    assert run.done and len(run.medium) <= 60
    for c, heard in enumerate(monitor(run)):
        assert {b"thirdone", S.PAY[0][c], S.PAY[1][c]} <= heard, c # both payloads decode
    first = [0 if a < b else 1 for a, b in zip(*run.starts)]
    assert set(first) == {0, 1}                                    # each station wins some channels
    for c in range(S.PAIRS):
        early, late = sorted((run.starts[0][c], run.starts[1][c]))
        assert late >= early + tones + S.T, c                      # the second begins after the first's tones are over
        loser = 1 - first[c]
        ticks = range(early // S.T, late // S.T + 1)
        assert any(run.busy[t][loser][c] for t in ticks), c        # it heard the first one ...
        assert sum(int(run.deferred[t][loser][c]) for t in ticks) > 0, c       # ... and moved its message for it


# --------------------------------------------------------------------- the Python layer's refusals (no device needed)

def bare_tx(n=4):
    tx = object.__new__(live.LiveTransmitter)
    tx.n_channels = n
    tx.device = "cpu"
    return tx


def test_pull_refuses_wrong_csma_arguments_before_anything_is_launched():
    tx = bare_tx()
    for kw in (dict(persist=63), dict(slot=4800), dict(seed=1), dict(slot=0), dict(seed=0)):    # given at all
        with pytest.raises(ValueError, match="need hold"):
            tx.pull(16, **kw)
    for kw, word in ((dict(persist=256), "persist"), (dict(persist=-1), "persist"), (dict(slot=-1), "slot"),
                     (dict(slot=2 ** 20 + 1), "slot"), (dict(seed=-1), "seed"), (dict(seed=2 ** 32), "seed")):
        with pytest.raises(ValueError, match=word):
            tx.pull(16, hold=False, **kw)


def test_push_refuses_a_wrong_mute_before_anything_is_launched():
    import torch
    n, T = 4, 64
    for bad in ([(0, 1)] * 3, np.zeros((n, 3), np.int32), np.zeros((n, 2), np.float32), [True] * 5, ["a"] * n):
        with pytest.raises(ValueError, match="mute"):
            live._device_mute(bad, n, T, torch.device("cpu"))
    got, up = live._device_mute([True, False, True, False], n, T, torch.device("cpu"))
    assert up and got.dtype == torch.int32 and got.tolist() == [[0, T], [0, 0], [0, T], [0, 0]]
    got, up = live._device_mute([(1, 2), (-7, 3), (5, 2 ** 40), (0, 0)], n, T, torch.device("cpu"))
    assert got.tolist() == [[1, 2], [-7, 3], [5, 2 ** 31 - 1], [0, 0]]
