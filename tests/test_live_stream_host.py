"""Host side of the streaming live receiver (no GPU): the block-by-block model (tests/live_stream_model.py) against the
CPU oracle at all 36 rates, the K-rule boundary included; the C-ABI declarations and their signature table;
afsk_live_stream_layout against its closed form and the per-channel bound; the argument checks that return before any
device is needed; and the Python constructor's checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from afskmodem_amd import _native, live
from oracle import afsk_oracle as O
from tests.live_stream_model import BLOCK, SYNC, StreamDemodModel, demod_streaming
from tests.stub_lib import arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_ENTRIES = ("afsk_live_stream_layout", "afsk_live_create_stream")
RX_BFS = tuple(bf for bf in range(4, 2048, 4) if 48000 % bf == 0)        # 36 rates: 12000 ... 24 baud
FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")


def oracle_demod(burst, bf, amp_end=14000, stride=512):
    r = O.demod_batch(burst, [0], [burst.size], [bf], amp_end, out_stride=stride)
    out = {f: int(r[f][0]) for f in FIELDS}
    out["bytes"] = r["bytes"][0, : min(out["nbytes"], stride)].tobytes()
    return out


def message(rng, bf, nbytes, lead=0, noise=0.0):
    """A modulated message at 48000 / bf baud (a short training), `lead` zero samples in front, optional noise."""
    baud = 48000 // bf
    data = bytes(rng.integers(0, 256, nbytes, dtype=np.uint8))
    f = O.get_frames(data, baud, max(0.02, 2.5 / baud)).astype(np.int16)
    if noise:
        f = np.clip(f + rng.normal(0, noise, f.size), -32768, 32767).astype(np.int16)
    return np.concatenate([np.zeros(lead, np.int16), f]), data


def whole_blocks(x, n_blocks):
    out = np.zeros(n_blocks * BLOCK, np.int16)
    m = min(x.size, out.size)
    out[:m] = x[:m]
    return out


def check(burst, bf, amp_end=14000):
    got = demod_streaming(burst, bf, amp_end, max_payload_len=512)
    want = oracle_demod(burst, bf, amp_end)
    for f in FIELDS:
        assert got[f] == want[f], (bf, f, got[f], want[f])
    assert got["bytes"] == want["bytes"], bf
    return got


@pytest.mark.parametrize("bf", RX_BFS)
def test_model_matches_the_oracle_on_random_bursts(bf):
    rng = np.random.default_rng(bf)
    sym = max(1, 3 * BLOCK // bf)
    for trial in range(3):
        nbytes = int(rng.integers(0, 6))
        x, _ = message(rng, bf, nbytes, lead=int(rng.integers(0, 64)), noise=[0.0, 3000.0, 9000.0][trial])
        # cut anywhere: mid-message, just past it, or with silence behind it
        n_blocks = max(1, int(rng.integers(1, -(-x.size // BLOCK) + 2)))
        if bf >= 1000:
            n_blocks = min(n_blocks, 12 + sym)
        check(whole_blocks(x, n_blocks), bf)


@pytest.mark.parametrize("bf", RX_BFS)
def test_model_k_rule_symbol_ending_at_the_last_sample(bf):
    """Trap 1: with ci + (k + 1) * bf == len the symbol k is not counted -- the burst must grow first."""
    rng = np.random.default_rng(1000 + bf)
    hits = 0
    for m in range(2, 90):
        length = m * BLOCK
        lead = length % bf
        if lead >= SYNC - 2 * bf or lead > 2 * BLOCK:
            continue
        x, _ = message(rng, bf, 2, lead=lead)
        burst = whole_blocks(x, m)
        ci = O.recover_clock_index(burst[:SYNC], 48000 // bf)
        if ci != lead:
            continue
        assert (length - ci) % bf == 0
        check(burst, bf)
        hits += 1
        if hits >= 2:
            break
    assert hits >= 1, bf


def test_model_short_and_no_terminator():
    """Traps 2 and 3: a one-block burst is TOO_SHORT; without a terminator the status is NO_DATA and term_frame is
    ci + K * bf."""
    rng = np.random.default_rng(5)
    x, _ = message(rng, 40, 4)
    got = check(whole_blocks(x, 1), 40)
    assert got["status"] == _native.ST_TOO_SHORT and got["clock_idx"] == -1 and got["term_frame"] == -1
    tr = np.tile(O.training_cycle(1200).astype(np.int16), 200)             # training only: no terminator
    for n_blocks in (2, 3, 5):
        got = check(whole_blocks(tr, n_blocks), 40)
        assert got["status"] == _native.ST_NO_DATA
        K = (n_blocks * BLOCK - got["clock_idx"] - 1) // 40
        assert got["term_frame"] == got["clock_idx"] + K * 40


def test_model_whole_codewords_and_truncated_rows():
    """Trap 4: ECC takes whole 7-bit codewords, bytes whole codeword pairs, nbits counts a partial codeword; a row
    longer than max_payload_len is truncated and nbytes stays the full count."""
    rng = np.random.default_rng(9)
    x, data = message(rng, 40, 40)
    for cut in range(6, 14):                        # bursts that end inside the data phase, loud to the end
        n_blocks = -(-x.size // BLOCK) - cut // 2
        check(whole_blocks(x, n_blocks), 40)
    full = whole_blocks(x, -(-x.size // BLOCK) + 1)
    got = demod_streaming(full, 40, max_payload_len=7)
    assert got["nbytes"] == 40 and got["bytes"] == data[:7]
    assert demod_streaming(full, 40, max_payload_len=0)["bytes"] == b""


def test_model_keeps_less_than_a_symbol_between_blocks():
    rng = np.random.default_rng(3)
    x, _ = message(rng, 160, 8)
    m = StreamDemodModel(160)
    burst = whole_blocks(x, -(-x.size // BLOCK) + 1)
    for b in range(burst.size // BLOCK):
        m.feed(burst[b * BLOCK:(b + 1) * BLOCK])
        if m.phase in (1, 2):
            assert m.keep.size <= 160                               # never more than a symbol once the clock is known
        elif m.phase == 0:
            assert m.keep.size == BLOCK


# ------------------------------------------------------------------------------------------------- C ABI (host)

def test_header_declares_stream_entries_in_their_own_table():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    for name in STREAM_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
        assert not re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.LIVE_STREAM_SIGNATURES) == set(STREAM_ENTRIES)
    for other in (_native.SIGNATURES, _native.SPLIT_SIGNATURES, _native.LIVE_SIGNATURES, _native.LIVE_TX_SIGNATURES,
                  _native.LIVE_MIXED_SIGNATURES):
        assert not set(STREAM_ENTRIES) & set(other)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    block = hdr[hdr.index("The streaming live receiver"):hdr.index("extern int afsk_live_stream_layout")]
    for line in ("a256(32 n) + a256(4096 n) + a256(32 n) + a256(4 n) + a256(8192 n)", "out_margins must be NULL",
                 "AFSK_ST_BAD_LENGTH", "AFSK_LIVE_OPEN_END", "capturable"):
        assert line in block, line


def test_library_exports_stream_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in STREAM_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2


def a256(x):
    return -(-x // 256) * 256


def closed_form(n, maxp):
    return a256(32 * n) + a256(4096 * n) + a256(32 * n) + a256(4 * n) + a256(8192 * n) + a256(maxp * n) + 256


@pytest.mark.parametrize("n", [1, 3, 64, 65536])
def test_stream_layout_closed_form_and_bound(n):
    for maxp, chunk in ((0, 1), (256, 8192), (13, 2048), (65536, 48000), (1000, 2049)):
        slots, nbytes = C.c_int32(-7), C.c_int64(-7)
        assert _native.lib().afsk_live_stream_layout(n, maxp, chunk, C.byref(slots), C.byref(nbytes)) == 0, \
            _native.last_error()
        k = (2047 + chunk) // 2048
        assert slots.value == 1 + k // 3
        assert nbytes.value == closed_form(n, maxp)
        assert nbytes.value <= n * (16384 + maxp + 256)                 # no burst length in it
        assert live.stream_layout(n, maxp, chunk) == (slots.value, nbytes.value)
        # the stored receiver's slots for the same chunk bound
        assert live.layout(n, 4096, chunk)[0] == slots.value
    # under 1/12 of the stored receiver's default (2 s bursts) per channel
    assert closed_form(n, 256) * 12 < live.layout(n, live.DEFAULT_MAX_BURST_LEN, 8192)[1]


@pytest.mark.parametrize("args", [(0, 256, 8192), (-1, 256, 8192), (4, -1, 8192), (4, 65537, 8192), (4, 256, 0),
                                  (4, 256, _native.MAX_STREAM_LEN + 1), (1 << 30, 256, 8192)])
def test_stream_layout_refusals(args):
    slots, nbytes = C.c_int32(-7), C.c_int64(-7)
    assert _native.lib().afsk_live_stream_layout(*args, C.byref(slots), C.byref(nbytes)) == _native.E_INVALID_ARG
    assert slots.value == -7 and nbytes.value == -7
    with pytest.raises(_native.AfskNativeError):
        live.stream_layout(*args)


@pytest.mark.parametrize("bad", [0, 6, 10, 41, 2048, -40])
def test_create_stream_refuses_a_bad_rate_in_any_channel(bad):
    for where in (0, 2, 4):
        a, p = arr([40, 160, 80, 20, 40])
        a[where] = bad
        h = C.c_void_p(1234)
        assert _native.lib().afsk_live_create_stream(5, p, 18000, 14000, 256, 8192, C.byref(h)) \
            == _native.E_INVALID_BAUD, (bad, where)
        assert not h


def test_create_stream_argument_checks():
    """Every refusal is an argument error, returned before the device check (AFSK_E_NO_DEVICE here)."""
    h = C.c_void_p(1234)
    a, p = arr([40, 160])
    assert _native.lib().afsk_live_create_stream(2, None, 18000, 14000, 256, 8192, C.byref(h)) == _native.E_INVALID_ARG
    assert not h
    for n in (0, -1):
        assert _native.lib().afsk_live_create_stream(n, p, 18000, 14000, 256, 8192, C.byref(h)) \
            == _native.E_INVALID_ARG
    assert _native.lib().afsk_live_create_stream(2, p, 18000, 14000, 256, 8192, None) == _native.E_INVALID_ARG
    for mp, mc in ((-1, 8192), (65537, 8192), (256, 0), (256, _native.MAX_STREAM_LEN + 1)):
        assert _native.lib().afsk_live_create_stream(2, p, 18000, 14000, mp, mc, C.byref(h)) == _native.E_INVALID_ARG
        assert not h
    if _native.device_count() == 0:
        assert _native.lib().afsk_live_create_stream(2, p, 18000, 14000, 256, 8192, C.byref(h)) \
            == _native.E_NO_DEVICE
        assert not h


def test_python_constructor_checks():
    with pytest.raises(Exception, match="Invalid baud rate"):
        live.LiveReceiver(4, 41, max_burst_len=None)
    with pytest.raises(_native.AfskNativeError):
        live.LiveReceiver(4, 40, max_burst_len=None, max_payload_len=65537)
    with pytest.raises(_native.AfskNativeError):
        live.LiveReceiver(0, 40, max_burst_len=None)
    if _native.device_count() == 0:
        with pytest.raises(_native.AfskNativeError) as e:
            live.LiveReceiver(4, [40, 160, 40, 20], max_burst_len=None)
        assert e.value.code == _native.E_NO_DEVICE
