"""Host side of the streaming receiver's payload tap (no GPU): the tap model (tests/live_tap_model.py) against the CPU
oracle -- the bytes committed per block, concatenated, are demod_batch's, and they are committed as soon as the K rule
allows; tap_cap against its closed form and against the model's worst pushes; the C-ABI declarations and their
signature table; the constructor's refusals; LiveResult.partials and PayloadAssembler on fabricated results."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from afskmodem_amd import _native, batch, live
from oracle import afsk_oracle as O
from tests.live_tap_model import BLOCK, TapChannelModel, TapDemodModel, tap_cap
from tests.stub_lib import arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAP_ENTRIES = ("afsk_live_tap_layout", "afsk_live_create_stream_tap", "afsk_live_push_tap")
# 6000, 2400, 1200, 300 and 24 baud, with a payload size that keeps the burst at a few hundred blocks
RATES = ((8, 3000), (20, 2000), (40, 1500), (160, 300), (2000, 12))


def frames(rng, bf, nbytes, lead=0, noise=0.0, training=None):
    baud = 48000 // bf
    data = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    f = O.get_frames(data, baud, max(0.02, 2.5 / baud) if training is None else training).astype(np.int16)
    if noise:
        f = np.clip(f + rng.normal(0, noise, f.size), -32768, 32767).astype(np.int16)
    return np.concatenate([np.zeros(lead, np.int16), f]), data


def whole_blocks(x, extra=1):
    out = np.zeros((-(-x.size // BLOCK) + extra) * BLOCK, np.int16)
    out[:x.size] = x
    return out


def oracle_bytes(burst, bf, amp_end=14000):
    stride = burst.size // (14 * bf) + 2
    r = O.demod_batch(burst, [0], [burst.size], [bf], amp_end, out_stride=stride)
    n = int(r["nbytes"][0])
    assert n <= stride
    return r["bytes"][0, :n].tobytes(), r


def run_model(burst, bf, amp_end=14000, maxp=0, each=None):
    m = TapDemodModel(bf, amp_end, maxp)
    parts = []
    for b in range(burst.size // BLOCK):
        parts.append(m.feed(burst[b * BLOCK:(b + 1) * BLOCK]))
        if each:
            each(m)
    return m, parts


def check_against_oracle(burst, bf, amp_end=14000):
    m, parts = run_model(burst, bf, amp_end)
    want, r = oracle_bytes(burst, bf, amp_end)
    assert b"".join(parts) == want, bf
    res = m.result()
    for f in ("nbytes", "nbits", "clock_idx", "term_frame", "status"):
        assert res[f] == int(r[f][0]), (bf, f)
    assert res["bytes"] == b"" and m.nbytes() == len(want)          # max_payload_len 0 truncates the row, not the tap
    return want


@pytest.mark.parametrize("bf,plen", RATES)
def test_committed_bytes_concatenate_to_the_oracles(bf, plen):
    rng = np.random.default_rng(bf)
    for noise in (0.0, 3000.0, 9000.0):
        n = int(rng.integers(plen // 2, plen + 1))
        x, data = frames(rng, bf, n, lead=int(rng.integers(0, min(64, bf))), noise=noise)
        got = check_against_oracle(whole_blocks(x), bf)
        if noise == 0.0:                                  # (noise may move the terminator: the oracle decides)
            assert got[:n] == data, (bf, noise)


def test_a_payload_longer_than_65536_bytes_at_6000_baud():
    rng = np.random.default_rng(66)
    x, data = frames(rng, 8, 66000, lead=3)
    got = check_against_oracle(whole_blocks(x), 8)
    assert len(data) > 65536 and got[:len(data)] == data


@pytest.mark.parametrize("bf", [8, 40, 160])
def test_false_terminator_squelch_stop_and_missing_terminator(bf):
    rng = np.random.default_rng(100 + bf)
    baud = 48000 // bf
    # a false terminator: a space symbol copied over a mark symbol of the training, past the clock search's samples
    x, _ = frames(rng, bf, 200, training=max(0.3, 40 * BLOCK / 48000 / 8))
    # (training symbols alternate: of the symbols k0 and k0 + 7 one is a space, and three copies of it behind it follow
    # a mark)
    for k in (4096 // bf + 9, 4096 // bf + 16):
        for j in (1, 2, 3):
            x[(k + j) * bf:(k + j + 1) * bf] = x[k * bf:(k + 1) * bf]
    m, parts = run_model(whole_blocks(x), bf)
    want, r = oracle_bytes(whole_blocks(x), bf)
    assert b"".join(parts) == want and m.result()["term_frame"] == int(r["term_frame"][0])
    assert m.result()["term_frame"] < 12000 and len(want) > 200     # decoding started inside the 14400-sample training
    # a squelch stop in mid-payload: silence from the middle of the data on
    x, data = frames(rng, bf, 400)
    cut = x.size - 200 * 14 * bf
    x[cut:] = 0
    got = check_against_oracle(whole_blocks(x, extra=3), bf)
    assert 150 < len(got) < 260 and got[:150] == data[:150]
    # no terminator: training only, and a message cut inside its training
    tr = np.tile(O.training_cycle(baud).astype(np.int16), 4 * BLOCK // (2 * bf) + 4)
    assert check_against_oracle(whole_blocks(tr)[:4 * BLOCK], bf) == b""
    x, _ = frames(rng, bf, 50, training=1.0)
    assert check_against_oracle(x[:8 * BLOCK].copy(), bf) == b""
    # too short for the clock search
    assert check_against_oracle(x[:BLOCK].copy(), bf) == b""


@pytest.mark.parametrize("bf,plen", RATES)
def test_bytes_are_committed_as_soon_as_the_k_rule_allows(bf, plen):
    """After every block: every symbol k with ci + (k + 1) * bf < len is committed, and so is every byte whose 14
    symbols are among them -- the prefix of the oracle's bytes of that length."""
    rng = np.random.default_rng(200 + bf)
    x, data = frames(rng, bf, plen // 3, lead=int(rng.integers(0, min(64, bf))), noise=1000.0)
    burst = whole_blocks(x)
    want, _ = oracle_bytes(burst, bf)
    seen = []

    def each(m):
        if m.phase in (1, 2):
            assert m.k == (m.length - m.ci - 1) // bf
        if m.phase == 2:
            assert len(m.tap) == (m.k - m.first) // 14
        assert bytes(m.tap) == want[:len(m.tap)]
        seen.append(len(m.tap))

    m, _ = run_model(burst, bf, each=each)
    assert seen[-1] == len(want) and len(want) > plen // 4
    assert sorted(seen) == seen and len(set(seen)) > 3             # delivered over many blocks, not at the end


# ----------------------------------------------------------------------------------------------------- tap_cap

def layout_cap(n, maxp, chunk, bf):
    cap = C.c_int32(-7)
    rc = _native.lib().afsk_live_tap_layout(n, maxp, chunk, bf, C.byref(cap))
    return rc, cap.value


@pytest.mark.parametrize("chunk", [1, 2047, 2048, 2049, 8192, 48000, _native.MAX_STREAM_LEN])
def test_tap_layout_is_the_headers_closed_form(chunk):
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    macro = re.search(r"#define AFSK_LIVE_TAP_CAP\(max_chunk_len, min_bit_frames\) \\\n\s*(.*)\n", hdr).group(1)
    expr = macro.replace("(int32_t)", "").replace("(int64_t)", "").replace("/", "//")
    for bf in (4, 8, 40, 160, 2000):
        k = (2047 + chunk) // 2048
        want = ((k + 1) * 2048 // bf) // 14 + 1
        assert tap_cap(chunk, bf) == want
        assert eval(expr, {"max_chunk_len": chunk, "min_bit_frames": bf}) == want
        assert layout_cap(64, 0, chunk, bf) == (0, want)
        assert live.tap_layout(3, 256, chunk, bf) == want
    assert _native.lib().afsk_live_tap_layout(4, 0, chunk, 40, None) == 0


@pytest.mark.parametrize("args", [(0, 256, 8192), (-1, 256, 8192), (4, -1, 8192), (4, 65537, 8192), (4, 256, 0),
                                  (4, 256, _native.MAX_STREAM_LEN + 1), (1 << 30, 256, 8192)])
def test_tap_layout_refuses_what_stream_layout_refuses(args):
    slots, nbytes = C.c_int32(), C.c_int64()
    assert _native.lib().afsk_live_stream_layout(*args, C.byref(slots), C.byref(nbytes)) == _native.E_INVALID_ARG
    assert layout_cap(*args, 40) == (_native.E_INVALID_ARG, -7)
    with pytest.raises(_native.AfskNativeError):
        live.tap_layout(*args, 40)


@pytest.mark.parametrize("bad", [0, 6, 41, 2048, -40])
def test_tap_layout_refuses_a_bad_rate(bad):
    assert layout_cap(4, 256, 8192, bad) == (_native.E_INVALID_BAUD, -7)


@pytest.mark.parametrize("T", [1, 2047, 2048, 2049, 8192, 48000])
@pytest.mark.parametrize("bf", [8, 40])
def test_tap_cap_bounds_the_models_worst_pushes(bf, T):
    """Continuous data from the second block of a burst on (the shortest training), the burst's first block arriving
    as the last block of a push or not (every alignment of the burst against the pushes): no push commits more than
    tap_cap bytes, and the worst push commits at least what K blocks of continuous data hold."""
    rng = np.random.default_rng(T + bf)
    cap = tap_cap(T, bf)
    k_blocks = (2047 + T) // 2048
    msg, _ = frames(rng, bf, (k_blocks + 1) * 3 * BLOCK // (14 * bf) + 40, training=2 * bf / 48000)
    worst = 0
    # alignments: a few fixed ones, and those that leave a carry of 2047 samples (a push of K blocks) at push j
    shifts = {0, 1, 7, BLOCK // 2} | {(BLOCK - 1 - j * T) % BLOCK for j in range(10)}
    for shift in sorted(shifts):
        for lead_blocks in range(1, 2 + min(k_blocks, 3)):
            stream = np.concatenate([np.zeros(lead_blocks * BLOCK, np.int16), msg])
            stream = stream[: (lead_blocks + 2 * k_blocks + 3) * BLOCK]
            ch = TapChannelModel(bf)
            ch.push(np.zeros(shift, np.int16))                       # the pushes' alignment against the blocks
            pushes = [stream[p:p + T] for p in range(0, stream.size, T)]
            if T < BLOCK:                                            # (only a push that completes a block commits)
                pushes = [stream[p:p + BLOCK] for p in range(0, stream.size, BLOCK)]
                pushes = [q for big in pushes for q in (big[:BLOCK - T], big[BLOCK - T:]) if q.size]
            for p in pushes:
                r = ch.push(p)
                if p.size <= T:
                    worst = max(worst, len(r["tap"]))
    assert 0 < worst <= cap, (worst, cap)
    assert worst >= (k_blocks * BLOCK // bf) // 14, (worst, cap)


# ------------------------------------------------------------------------------------------------- C ABI (host)

def test_header_declares_tap_entries_in_their_own_table():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    for name in TAP_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
        assert not re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert hdr.index("extern int " + name) > hdr.index("extern int afsk_live_create_stream(")
    assert set(_native.LIVE_TAP_SIGNATURES) == set(TAP_ENTRIES)
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "LIVE_TAP_SIGNATURES"]
    assert len(others) >= 8
    for other in others:
        assert not set(TAP_ENTRIES) & set(other)
    assert set(_native.LIVE_STREAM_SIGNATURES) == {"afsk_live_stream_layout", "afsk_live_create_stream"}
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    # afsk_live_push's arguments and the five tap outputs
    tap_args = _native.LIVE_TAP_SIGNATURES["afsk_live_push_tap"][1]
    assert len(tap_args) == len(_native.LIVE_SIGNATURES["afsk_live_push"][1]) + 5


def test_library_exports_tap_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in TAP_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2


def test_create_and_push_argument_checks_before_any_device():
    lib = _native.lib()
    h = C.c_void_p(1234)
    (_, bf), (_, s), (_, e) = arr([40, 160]), arr([18000, 18000]), arr([14000, 9000])
    assert lib.afsk_live_create_stream_tap(2, None, s, e, 0, 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert not h
    assert lib.afsk_live_create_stream_tap(2, bf, None, e, 0, 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert lib.afsk_live_create_stream_tap(2, bf, s, None, 0, 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert lib.afsk_live_create_stream_tap(2, bf, s, e, 0, 8192, None) == _native.E_INVALID_ARG
    for n in (0, -1):
        assert lib.afsk_live_create_stream_tap(n, bf, s, e, 0, 8192, C.byref(h)) == _native.E_INVALID_ARG
    for mp, mc in ((-1, 8192), (65537, 8192), (0, 0), (0, _native.MAX_STREAM_LEN + 1)):
        assert lib.afsk_live_create_stream_tap(2, bf, s, e, mp, mc, C.byref(h)) == _native.E_INVALID_ARG
        assert not h
    _, bad = arr([40, 41])
    assert lib.afsk_live_create_stream_tap(2, bad, s, e, 0, 8192, C.byref(h)) == _native.E_INVALID_BAUD
    if _native.device_count() == 0:
        assert lib.afsk_live_create_stream_tap(2, bf, s, e, 0, 8192, C.byref(h)) == _native.E_NO_DEVICE
        assert not h
    null_push = [None, None, 0, 0, 0] + [None] * 5 + [0] + [None] * 7 + [0] + [None] * 6
    assert lib.afsk_live_push_tap(*null_push) == _native.E_INVALID_ARG                  # a null receiver


def test_python_constructor_checks():
    with pytest.raises(ValueError, match="progressive"):
        live.LiveReceiver(4, 40, progressive=True)                              # a stored receiver
    with pytest.raises(ValueError, match="progressive"):
        live.LiveReceiver(4, 40, max_burst_len=48000, progressive=True)
    with pytest.raises(_native.AfskNativeError):
        live.LiveReceiver(4, 40, max_burst_len=None, max_payload_len=65537, progressive=True)
    with pytest.raises(_native.AfskNativeError):
        live.LiveReceiver(0, 40, max_burst_len=None, progressive=True)
    if _native.device_count() == 0:
        with pytest.raises(_native.AfskNativeError) as e:
            live.LiveReceiver(4, [40, 160, 40, 20], max_burst_len=None, max_payload_len=0, progressive=True)
        assert e.value.code == _native.E_NO_DEVICE
    r = live.LiveResult(None, None, np.zeros((1, 2), np.int32), None, None)
    assert r.tap is None
    with pytest.raises(ValueError, match="progressive"):
        r.partials()


# ------------------------------------------------------------------------- partials and the assembler (fabricated)

SLOTS, CAP = 3, 16


def fabricate(n, closed=(), open_=(), overflow=()):
    """A LiveResult of numpy arrays for n channels.  closed: (channel, start, length, nbytes, data) per reported burst
    in time order; open_: (channel, start, nbytes so far, data)."""
    nc = np.zeros(n, np.int32)
    bs, bl, fl = np.zeros((n, SLOTS), np.int64), np.zeros((n, SLOTS), np.int32), np.zeros((n, SLOTS), np.int32)
    nbytes = np.zeros(n * SLOTS, np.int32)
    tb, tn, tl = np.full((n, CAP), 0xEE, np.uint8), np.zeros(n, np.int32), np.zeros((n, SLOTS), np.int32)
    os_, on = np.full(n, -1, np.int64), np.zeros(n, np.int32)
    for c, start, length, nb, data in closed:
        k = int(nc[c])
        bs[c, k], bl[c, k], nbytes[c * SLOTS + k], tl[c, k] = start, length, nb, len(data)
        if (c, start) in overflow:
            fl[c, k] = _native.LIVE_OVERFLOW
        tb[c, tn[c]:tn[c] + len(data)] = np.frombuffer(data, np.uint8)
        tn[c] += len(data)
        nc[c] += 1
    for c, start, nb, data in open_:
        os_[c], on[c] = start, nb
        tb[c, tn[c]:tn[c] + len(data)] = np.frombuffer(data, np.uint8)
        tn[c] += len(data)
    z = np.zeros(n * SLOTS, np.int32)
    demod = batch.DemodResult(np.zeros((n * SLOTS, 0), np.uint8), nbytes, z, z, z, z)
    return live.LiveResult(nc, bs, bl, fl, demod, live.LiveTap(tb, tn, tl, os_, on))


def test_partials_several_bursts_of_one_channel_in_one_push():
    r = fabricate(3, closed=[(1, 2048, 6144, 5, b"llo w"), (1, 12288, 4096, 3, b"abc"), (2, 0, 4096, 0, b"")],
                  open_=[(1, 20480, 2, b"xy"), (0, 4096, 0, b"")])
    assert r.partials() == [(1, 2048, 0, b"llo w", True), (1, 12288, 0, b"abc", True), (1, 20480, 0, b"xy", False),
                            (2, 0, 0, b"", True)]
    asm = live.PayloadAssembler()
    assert asm.feed(r) == [(1, 2048, 6144, b"llo w"), (1, 12288, 4096, b"abc"), (2, 0, 4096, b"")]
    assert asm.pending() == {1: (20480, b"xy")}


def test_assembler_a_burst_over_many_pushes_a_close_without_new_bytes_and_flush():
    asm = live.PayloadAssembler(string=True)
    text = "progressive payloads arrive early"
    data = text.encode()
    at = 0
    for step in (4, 0, 9, 7, 0, 13):
        r = fabricate(2, open_=[(0, 4096, at + step, data[at:at + step])])
        assert r.partials() == ([(0, 4096, at, data[at:at + step], False)] if step else [])
        assert asm.feed(r) == []
        at += step
        assert asm.pending() == {0: (4096, data[:at])}
    assert at == len(data)
    # the burst closes in a push that decodes nothing more: one final event with b""
    r = fabricate(2, closed=[(0, 4096, 40960, len(data), b"")])
    assert r.partials() == [(0, 4096, len(data), b"", True)]
    assert asm.feed(r) == [(0, 4096, 40960, text)]
    assert asm.pending() == {}
    # a flush reports the open burst in a slot (with its last bytes), nothing stays open
    asm = live.PayloadAssembler()
    asm.feed(fabricate(2, open_=[(1, 8192, 3, b"abc")]))
    r = fabricate(2, closed=[(1, 8192, 6144, 5, b"de")])
    assert r.partials() == [(1, 8192, 3, b"de", True)]
    assert asm.feed(r) == [(1, 8192, 6144, b"abcde")]
    # a missing push is noticed
    asm.feed(fabricate(2, open_=[(1, 8192, 3, b"abc")]))
    with pytest.raises(ValueError, match="missing or out of order"):
        asm.feed(fabricate(2, open_=[(1, 8192, 9, b"hi")]))


def test_assembler_a_reset_channel_and_an_overflowed_burst():
    asm = live.PayloadAssembler()
    asm.feed(fabricate(3, open_=[(0, 4096, 3, b"abc"), (2, 2048, 2, b"zz")]))
    assert set(asm.pending()) == {0, 2}
    # channel 0 was reset: nothing of it is recording after the next push, channel 2 goes on
    assert asm.feed(fabricate(3, open_=[(2, 2048, 3, b"z")])) == []
    assert asm.pending() == {2: (2048, b"zzz")}
    # a new burst of channel 0 (its stream restarted) is assembled from offset 0
    r = fabricate(3, closed=[(0, 2048, 4096, 2, b"ok")], open_=[(2, 2048, 3, b"")])
    assert asm.feed(r) == [(0, 2048, 4096, b"ok")]
    # drop() mirrors reset(mask) on the host at once
    asm.drop(np.array([0, 0, 1], bool))
    assert asm.pending() == {}
    # an overflowed burst: b"", as bursts() reports it, whatever was handed out before
    asm.feed(fabricate(1, open_=[(0, 4096, 4, b"abcd")]))
    r = fabricate(1, closed=[(0, 4096, 2147481600, 0, b"")], overflow={(0, 4096)})
    assert asm.feed(r) == [(0, 4096, 2147481600, b"")]
    assert asm.pending() == {}
