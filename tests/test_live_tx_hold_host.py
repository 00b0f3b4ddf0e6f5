"""Host side of carrier sense on the live side (no GPU): the C-ABI declarations of afsk_live_busy and
afsk_live_tx_pull_hold, their signature table and the library's exports; the hold model
(tests/live_tx_hold_model.py) against hand-worked cases and its two properties -- no hold and no holdoff is the base
model, and a held-then-released stream is the unheld stream with ``sum(deferred)`` zeros put in where it was deferred;
the busy model against the bursts the reference's ``__listen`` recorded (tests/golden/); and the refusals of
``LiveTransmitter.pull(hold=)`` / ``LiveReceiver.busy(out=)`` that need no device."""
import ctypes as C
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from tests import live_tx_hold_model as H
from tests.golden_inputs import build_capture, listen_cases
from tests.live_tx_model import LiveTxModel
from tests.live_tx_rated_model import LiveTxRatedModel
from tests.test_live_ragged_host import declared_args, header

ENTRIES = ("afsk_live_busy", "afsk_live_tx_pull_hold")
TR = afskmodem.Transmitter(1200, 0.0)            # a message of p bytes: 40 * (4 + 14 p) + 4800 samples


def test_header_declares_the_entries_in_their_own_table():
    hdr = header()
    assert set(_native.LIVE_TX_HOLD_SIGNATURES) == set(ENTRIES)
    for name in ENTRIES:
        res, args = _native.LIVE_TX_HOLD_SIGNATURES[name]
        assert res is C.c_int and args == declared_args(hdr, name), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_tx_submit_events_rated(")
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_TX_HOLD_SIGNATURES"]
    assert len(others) >= 16 and all(not set(ENTRIES) & set(o) for o in others)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    # the ragged pull's arguments with hold and holdoff behind lens and out_deferred behind out_pending
    ragged = _native.LIVE_RAGGED_SIGNATURES["afsk_live_tx_pull_ragged"][1]
    hold = _native.LIVE_TX_HOLD_SIGNATURES["afsk_live_tx_pull_hold"][1]
    assert hold[:5] + [hold[7]] + [hold[9]] == ragged and hold[5] is C.c_void_p and hold[6] is C.c_int32
    for word in ("earliest", "holdoff", "p-persistence"):
        assert word in hdr


def test_library_exports_and_binds_the_entries():
    raw = C.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert getattr(_native.lib(), name).argtypes == _native.LIVE_TX_HOLD_SIGNATURES[name][1]
    assert _native.lib().afsk_version() == 2


def test_null_handles_are_refused_before_a_device_is_needed():
    lib = _native.lib()
    assert lib.afsk_live_busy(None, None, None) == _native.E_INVALID_ARG
    assert "null live receiver" in _native.last_error()
    assert lib.afsk_live_tx_pull_hold(None, None, 0, 0, None, None, 0, None, None, None) == _native.E_INVALID_ARG
    assert "null live transmitter" in _native.last_error()


# ------------------------------------------------------------------------------------------------ the hold model

def model(n=1, depth=4, wav=True):
    return H.HoldTxModel(n, 40, 0, depth, 64, wav=TR.wav_samples if wav else None)


def test_hand_worked_hold_and_holdoff():
    # b"" is 4960 samples, b"a" 5520
    m = model()
    st, s, _ = m.submit([0, 0], [b"", b"a"])
    assert s.tolist() == [0, 4960]
    # held while idle: u = the first message (start == pos), delta = L; both move, back to back
    out, pend, dfr = m.pull_hold(1000, hold=[1], holdoff=300)
    assert not out.any() and pend.tolist() == [2] and dfr.tolist() == [1000]
    assert list(m.queue[0]) == [(1000, 4960), (5960, 5520)] and m.end[0] == 11480 and m.wait == [300]
    # released: the wait of 300 samples is served inside this pull, the message begins 300 samples in
    out, pend, dfr = m.pull_hold(1000, hold=[0], holdoff=300)
    assert dfr.tolist() == [300] and not out[0, :300].any() and (out[0, 300:] == TR.wav_samples(b"")[:700]).all()
    assert list(m.queue[0]) == [(1300, 4960), (6260, 5520)] and m.wait == [0]
    # held while the first message is on air: it plays on, its successor (start 6260 inside the pull) moves to the end
    out, pend, dfr = m.pull_hold(5000, hold=[1], holdoff=10000)
    assert dfr.tolist() == [7000 - 6260] and (out[0, :4260] == TR.wav_samples(b"")[700:]).all() and not out[0, 4260:].any()
    assert list(m.queue[0]) == [(7000, 5520)] and pend.tolist() == [1] and m.wait == [10000]
    # a plain pull of the base model in between leaves w alone (and plays whatever is due: nothing before 7000 + ...)
    assert m.pull(0).tolist() == [1] and m.wait == [10000]
    # released with a wait longer than the pull: nothing begins, w counts down by L
    out, pend, dfr = m.pull_hold(4000, hold=None, holdoff=0)
    assert dfr.tolist() == [10000] and not out.any() and m.wait == [6000] and list(m.queue[0]) == [(17000, 5520)]
    # the message is now beyond the wait: deferred 0 although w > 0
    out, pend, dfr = m.pull_hold(4000)
    assert dfr.tolist() == [0] and m.wait == [2000] and not out.any()
    # a submit queues behind the shifted end
    st, s, _ = m.submit([0], [b""])
    assert s.tolist() == [17000 + 5520] and m.end[0] == 17000 + 5520 + 4960
    # L = 0 with hold: the wait is set, nothing moves
    out, pend, dfr = m.pull_hold(4000, lens=[0], hold=[1], holdoff=77, fill=9)
    assert dfr.tolist() == [0] and m.wait == [77] and (out == 9).all() and m.pos == [15000]
    m.reset([True])
    assert m.wait == [0] and m.pos == [0]


def test_a_message_wholly_beyond_the_pull_is_not_deferred_and_on_air_messages_are_never_touched():
    m = model()
    m.submit([0], [b"abc"])
    m.pull_hold(100)                                          # on air: start 0 < pos
    out, pend, dfr = m.pull_hold(3000, hold=[1], holdoff=5)
    assert dfr.tolist() == [0] and (out[0] == TR.wav_samples(b"abc")[100:3100]).all()
    assert list(m.queue[0]) == [(0, 40 * 46 + 4800)]


def script(seed, n, pulls):
    rng = np.random.default_rng(seed)
    for _ in range(pulls):
        T = int(rng.choice([1, 700, 2048, 4099, 9000]))
        k = int(rng.integers(0, 4))
        yield T, sorted(rng.integers(0, n, k).tolist()), [bytes(rng.integers(0, 256, int(rng.integers(0, 5)),
                                                                             dtype=np.uint8)) for _ in range(k)], rng


def test_no_hold_and_no_holdoff_is_the_base_model():
    n = 3
    base, hold = LiveTxModel(n, 40, 0, 3, 64, wav=TR.wav_samples), model(n, 3)
    for T, chans, pays, rng in script(5, n, 60):
        for a, b in zip(base.submit(chans, pays), hold.submit(chans, pays)):
            assert (a == b).all()
        want = base.expected(T)
        out, pend, dfr = hold.pull_hold(T, hold=[0] * n if rng.random() < 0.5 else None, holdoff=0)
        assert (out == want).all() and (pend == base.pull(T)).all() and not dfr.any()
        assert hold.pos == base.pos and hold.end == base.end and hold.wait == [0] * n
    # the rated model, ragged: a message's samples are its table entry + 1 throughout (the queue is what is tested)
    table = [(40, 0), (160, 3)]
    wav = lambda p, e: np.full(table[e][0] * (2 * table[e][1] + 4 + 14 * len(p)) + 4800, e + 1, np.int16)  # noqa: E731
    rated, held = LiveTxRatedModel(2, table, 3, 8, wav=wav), H.HoldTxRatedModel(2, table, 3, 8, wav=wav)
    for mdl in (rated, held):
        mdl.submit([0, 0, 1], [b"a", b"bc", b""], [1, 0, 1])
    for T in (3000, 9000, 9000, 30000):
        lens = [T, T // 2]
        want = rated.expected_ragged(T, lens, 7)
        out, pend, dfr = held.pull_hold(T, lens=lens, fill=7)
        assert (out == want).all() and want.any()
        assert (pend == rated.pull_ragged(T, lens)).all() and not dfr.any() and held.pos == rated.pos


def test_a_held_then_released_stream_is_the_unheld_stream_with_the_deferred_zeros_put_in():
    rng = np.random.default_rng(12)
    for trial in range(20):
        held = model(1, 4)
        pays = [bytes(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8)) for _ in range(3)]
        held.submit([0, 0, 0], pays)
        total = sum(TR.wav_samples(p).size for p in pays)
        stream_free = np.concatenate([TR.wav_samples(p) for p in pays])
        holdoff = int(rng.choice([0, 1, 4097, 6000]))
        got, cuts = [], []                                    # cuts: (index in the UNHELD stream, zeros inserted)
        shifted = 0
        hold_ticks = {0} | set(rng.choice(12, int(rng.integers(1, 6)), replace=False).tolist())   # (0: start == pos)
        t = 0
        while held.pending().any() or t < 12:
            T = int(rng.choice([500, 2048, 4099]))
            h = [1] if t in hold_ticks else [0]
            q = list(held.queue[0])
            u = next((s for s, _ in q if s >= held.pos[0]), None)
            out, _, dfr = held.pull_hold(T, hold=h, holdoff=holdoff)
            if dfr[0]:
                cuts.append((u - shifted, int(dfr[0])))       # u's start in the unheld stream
                shifted += int(dfr[0])
            got.append(out[0])
            t += 1
            assert t < 400
        got = np.concatenate(got)
        assert cuts and shifted == sum(z for _, z in cuts)
        want, at = [], 0
        for where, zeros in cuts:
            want += [stream_free[at:where], np.zeros(zeros, np.int16)]
            at = where
        want = np.concatenate(want + [stream_free[at:]])
        assert want.size == total + shifted
        assert (got[: want.size] == want).all() and not got[want.size:].any(), trial


# ------------------------------------------------------------------------------------------------ the busy model

def test_busy_model_against_the_bursts_the_reference_recorded(golden):
    cases = listen_cases(golden)
    assert len(cases) >= 19
    seen_busy = seen_free = 0
    for c in cases:
        cap = build_capture(c["recipe"])
        m = H.BusyModel(c["amp_start"], c["amp_end"])
        bursts = [(b["start"], b["len"]) for b in c["bursts"]]
        for P in range(0, cap.size // H.BLOCK * H.BLOCK + 1, H.BLOCK):
            if P:
                m.push(cap[P - H.BLOCK: P])
            want = any(s < P < s + n for s, n in bursts)
            if c["open_end"] and bursts and P >= bursts[-1][0] + bursts[-1][1]:
                want = True                                   # never closed: recording to the end of the capture
            assert m.busy == int(want), (c["name"], P)
            seen_busy += want
            seen_free += not want
        # the chunking does not matter: sample by sample in odd pieces, the same answers at the same positions
        m2, p = H.BusyModel(c["amp_start"], c["amp_end"]), 0
        for t in (1, 2047, 2049, 5000, 3, 10 ** 9):
            m2.push(cap[p: p + t])
            p = min(p + t, cap.size)
            P = p // H.BLOCK * H.BLOCK
            want = any(s < P < s + n for s, n in bursts) or \
                bool(c["open_end"] and bursts and P >= bursts[-1][0] + bursts[-1][1])
            assert m2.busy == int(want), (c["name"], p)
    assert seen_busy > 50 and seen_free > 50


def test_busy_model_hand_worked_and_flush():
    loud, quiet = np.full(H.BLOCK, 20000, np.int16), np.zeros(H.BLOCK, np.int16)
    m = H.BusyModel()
    assert m.push(loud) == 0                                  # the discarded block (ref:303)
    assert m.push(loud[:2047]) == 0 and m.push(loud[:1]) == 1  # a whole block above amp_start: recording
    assert m.push(loud) == 1 and m.push(quiet) == 0           # the first block below amp_end ends it
    assert m.push(loud) == 0 and m.push(loud) == 1            # the next __listen discards a block again
    assert m.push(quiet[:5], flush=True) == 0 and m.pos == 0
    assert H.busy_after(np.concatenate([quiet, loud, loud, quiet]), [4096, 2048, 2048]) == [1, 1, 0]
    edge = np.full(H.BLOCK, 18000, np.int16)                  # amp == amp_start: not above
    assert H.busy_after(np.concatenate([quiet, edge, loud, np.full(H.BLOCK, 14000, np.int16), quiet]),
                        [2048] * 5) == [0, 0, 1, 1, 0]        # amp == amp_end: not below


# --------------------------------------------------------------------- the Python layer's refusals (no device needed)

def bare_tx(n=4):
    tx = object.__new__(live.LiveTransmitter)
    tx.n_channels = n
    tx.device = "cpu"
    return tx


def test_pull_refuses_a_wrong_hold_before_anything_is_launched():
    tx = bare_tx()
    with pytest.raises(ValueError, match="holdoff needs hold"):
        tx.pull(16, holdoff=5)
    with pytest.raises(ValueError, match="holdoff"):
        tx.pull(16, hold=False, holdoff=-1)
    with pytest.raises(ValueError, match="holdoff"):
        tx.pull(16, hold=False, holdoff=_native.MAX_STREAM_LEN + 1)
    with pytest.raises(ValueError, match=r"n_channels=4"):
        tx.pull(16, hold=[1, 0, 1])
    with pytest.raises(ValueError, match=r"n_channels=4"):
        tx.pull(16, hold=np.zeros((4, 1), np.int32))
    with pytest.raises(ValueError, match="bool or integer"):
        tx.pull(16, hold=[0.5, 0.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="bool or integer"):
        tx.pull(16, hold=["a", "b", "c", "d"])
