"""Host side of the live receiver (no GPU): the C-ABI declarations and exports, afsk_live_layout against a closed
form and its argument checks, a pure-Python model of the chunked gate walk -- the slot bound over random amplitude
sequences and chunkings, reached exactly, and agreement with the oracle's whole-capture gate -- and the
no-device error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, live
from oracle import afsk_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_ENTRIES = ("afsk_live_layout", "afsk_live_create", "afsk_live_info", "afsk_live_push", "afsk_live_reset",
                "afsk_live_destroy")
BLOCK = 2048


def test_header_declares_live_entries():
    hdr = open(os.path.join(ROOT, "include", "afsk_amd.h")).read()
    assert "typedef struct afsk_live afsk_live;" in hdr
    for name in LIVE_ENTRIES:
        assert re.search(r"^extern int %s\(" % name, hdr, flags=re.M), name
    assert set(_native.LIVE_SIGNATURES) == set(LIVE_ENTRIES)
    assert not set(_native.LIVE_SIGNATURES) & set(_native.SIGNATURES)
    assert not set(_native.LIVE_SIGNATURES) & set(_native.SPLIT_SIGNATURES)
    assert int(re.search(r"#define AFSK_ABI_VERSION (\d+)", hdr).group(1)) == 2
    assert int(re.search(r"#define AFSK_LIVE_OPEN_END (\d+)", hdr).group(1)) == _native.LIVE_OPEN_END
    assert int(re.search(r"#define AFSK_LIVE_OVERFLOW (\d+)", hdr).group(1)) == _native.LIVE_OVERFLOW


def test_library_exports_live_entries():
    lib = C.CDLL(_native.LIB_PATH)
    for name in LIVE_ENTRIES:
        assert getattr(lib, name) is not None
    assert _native.lib().afsk_version() == 2        # binds all three tables


def a256(x):
    return -(-x // 256) * 256


def closed_form(n, max_burst_len, max_chunk_len):
    k = (2047 + max_chunk_len) // BLOCK
    slots = 1 + k // 3
    row = (max_burst_len // BLOCK + k) * BLOCK
    nbytes = a256(32 * n) + a256(2 * BLOCK * n) + a256(8 * n * slots) + a256(4 * n * slots) + a256(2 * row * n) + 256
    return slots, nbytes


def c_layout(n, mb, mc):
    slots, nbytes = C.c_int32(-7), C.c_int64(-7)
    rc = _native.lib().afsk_live_layout(n, mb, mc, C.byref(slots), C.byref(nbytes))
    return rc, int(slots.value), int(nbytes.value)


@pytest.mark.parametrize("n", [1, 3, 64, 65536])
def test_layout_closed_form(n):
    for mb in (4096, 5000, 96000, 192000, _native.MAX_STREAM_LEN):
        for mc in (1, 2047, 2048, 2049, 6143, 6144, 6145, 8192, 48000, 1 << 20, _native.MAX_STREAM_LEN):
            rc, slots, nbytes = c_layout(n, mb, mc)
            if n * closed_form(n, mb, mc)[0] > 2 ** 31 - 1:      # the demodulator's stream count is int32
                assert rc == _native.E_INVALID_ARG, (mb, mc)
                continue
            assert rc == 0, _native.last_error()
            assert (slots, nbytes) == closed_form(n, mb, mc), (mb, mc)
            assert live.layout(n, mb, mc) == (slots, nbytes)


@pytest.mark.parametrize("args", [(0, 96000, 8192), (-1, 96000, 8192), (4, 4095, 8192), (4, 0, 8192),
                                  (4, _native.MAX_STREAM_LEN + 1, 8192), (4, 96000, 0), (4, 96000, -5),
                                  (4, 96000, _native.MAX_STREAM_LEN + 1), (1 << 30, 96000, 48000)])
def test_layout_refuses_bad_arguments(args):
    rc, slots, nbytes = c_layout(*args)
    assert rc == _native.E_INVALID_ARG and (slots, nbytes) == (-7, -7)
    with pytest.raises(_native.AfskNativeError) as ei:
        live.layout(*args)
    assert ei.value.code == _native.E_INVALID_ARG


def test_entries_refuse_null_handles_without_a_device():
    lib = _native.lib()
    assert lib.afsk_live_create(4, 40, 18000, 14000, 96000, 8192, None) == _native.E_INVALID_ARG
    h = C.c_void_p()
    assert lib.afsk_live_create(4, 41, 18000, 14000, 96000, 8192, C.byref(h)) == _native.E_INVALID_BAUD and not h
    assert lib.afsk_live_create(4, 40, 18000, 14000, 100, 8192, C.byref(h)) == _native.E_INVALID_ARG and not h
    assert lib.afsk_live_info(None, None, None, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_push(None, None, 0, 0, 0, *([None] * 5), 0, *([None] * 7), 0, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_reset(None, None, None) == _native.E_INVALID_ARG
    assert lib.afsk_live_destroy(None) == 0


# ------------------------------------------------------------------------------------------------ the walk, modelled

class Model:
    """The chunked gate of live_gate_kernel over per-block amplitudes: amp(b) is the amplitude of stream block b
    (only asked for once the block is complete).  push(T) -> [(start, len, flags)] reported in that push."""

    def __init__(self, amp, amp_start=18000, amp_end=14000):
        self.amp = amp
        self.amp_start, self.amp_end = amp_start, amp_end
        self.pos = self.mode = self.rec_start = self.rec_len = 0

    def push(self, T, flush=False):
        out = []
        first = self.pos // BLOCK
        last = (self.pos + T) // BLOCK                  # blocks [first, last) complete in this push
        for b in range(first, last):
            a = self.amp(b)
            if self.mode == 0:
                self.mode = 1
            elif self.mode == 1:
                if a > self.amp_start:
                    self.mode, self.rec_start, self.rec_len = 2, b * BLOCK, BLOCK
            else:
                self.rec_len += BLOCK
                if a < self.amp_end:
                    out.append((self.rec_start, self.rec_len, 0))
                    self.mode = 0
        self.pos += T
        if flush:
            if self.mode == 2:
                out.append((self.rec_start, self.rec_len, _native.LIVE_OPEN_END))
            self.pos = self.mode = 0
        return out


def chunking(rng, total, mc):
    """Random push sizes 0 ... mc summing to total, with the edge sizes mixed in."""
    edges = [0, 1, 2047, 2049, mc, 2048]
    sizes, left = [], total
    while left > 0:
        t = int(rng.choice(edges)) if rng.random() < 0.4 else int(rng.integers(0, mc + 1))
        t = min(t, mc, left)
        sizes.append(t)
        left -= t
    return sizes


@pytest.mark.parametrize("mc", [1, 2047, 2048, 2049, 4096, 6143, 6144, 6145, 8192, 12289, 20000])
def test_walk_never_exceeds_the_slots(mc):
    slots, _ = closed_form(1, 96000, mc)
    assert c_layout(1, 96000, mc)[1] == slots
    rng = np.random.default_rng(mc)
    most = 0
    for trial in range(300):
        nb = int(rng.integers(0, 60 if mc >= 2047 else 5))       # (T = 1: a push per sample)
        # loud / quiet / in between, with runs that close a burst every third block
        amps = rng.choice([0, 16000, 20000, 30000], nb, p=[0.35, 0.1, 0.25, 0.3]) if trial % 3 else \
            np.resize(np.array([30000, 30000, 0]), nb)
        model = Model(lambda b: int(amps[b]))
        total = nb * BLOCK + int(rng.integers(0, BLOCK))
        sizes = chunking(rng, total, mc)
        for i, t in enumerate(sizes):
            got = model.push(t, flush=(i == len(sizes) - 1))
            assert len(got) <= slots, (mc, trial, t)
            most = max(most, len(got))
    assert most <= slots


@pytest.mark.parametrize("mc", [1, 2048, 2049, 4095, 4096, 6143, 6144, 6145, 8191, 8192, 12289, 48000, 65536])
def test_slot_bound_is_reached(mc):
    """For every K some push fills every slot: a burst open from the previous push with a 2047-sample carry closes
    in the first block, then discard / start / end triples; when K % 3 == 0 a flush adds the burst still open."""
    slots, _ = closed_form(1, 96000, mc)
    k = (2047 + mc) // BLOCK
    # blocks 0 discard, 1 start; a push ending 2047 samples into the block after them leaves the burst open
    pattern = {0: 0, 1: 30000, 2: 0}
    for i in range(1, k):
        pattern[2 + i] = (30000, 30000, 0)[(i - 1) % 3]
    model = Model(lambda b: pattern.get(b, 0))
    pre = 2 * BLOCK + 2047
    while pre > 0:                                      # reach that state with pushes of at most mc
        t = min(pre, mc)
        assert model.push(t) == []
        pre -= t
    assert model.mode == 2 and model.pos % BLOCK == 2047
    got = model.push(mc, flush=(k % 3 == 0))
    assert len(got) == slots, (mc, k, got)
    assert got[0] == (BLOCK, 2 * BLOCK, 0)


def capture_from_blocks(rng, amps, tail):
    """Samples whose block b has amplitude amps[b] exactly (alternating +-a), plus a partial block."""
    x = np.concatenate([np.tile(np.array([a, -a], np.int16), BLOCK // 2) for a in amps] +
                       [rng.integers(-32768, 32768, tail).astype(np.int16)])
    return x.astype(np.int16)


def test_model_matches_the_oracle_gate_on_whole_captures():
    rng = np.random.default_rng(5)
    for trial in range(400):
        nb = int(rng.integers(0, 40))
        amps = rng.choice([0, 5000, 14000, 16000, 18000, 18001, 25000], nb)
        cap = capture_from_blocks(rng, amps, int(rng.integers(0, BLOCK)))
        block_amp = [O.get_amplitude(cap[BLOCK * b: BLOCK * b + BLOCK]) for b in range(len(cap) // BLOCK)]
        want, want_oe = O.gate_stream(cap, 18000, 14000, 64)
        mc = int(rng.choice([1, 2047, 2049, 3000, 8192] if nb < 4 else [2047, 2049, 3000, 8192]))
        model = Model(lambda b: block_amp[b])
        got = []
        sizes = chunking(rng, len(cap), mc)
        for i, t in enumerate(sizes or [0]):
            got += model.push(t, flush=(i == len(sizes or [0]) - 1))
        assert [(s, n) for s, n, _ in got] == want, trial
        assert [f for _, _, f in got] == [0] * (len(want) - want_oe) + [_native.LIVE_OPEN_END] * want_oe, trial


def test_live_receiver_needs_a_device():
    """Without a GPU the live receiver raises the package's no-device error; there is no CPU stand-in."""
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_native.AfskNativeError) as ei:
        afskmodem.LiveReceiver(4, 40)
    assert ei.value.code == _native.E_NO_DEVICE and "no HIP device" in str(ei.value)
    with pytest.raises(_native.AfskNativeError) as ei:
        afskmodem.Receiver(1200).live(4, max_chunk_len=2048)
    assert ei.value.code == _native.E_NO_DEVICE
    h = C.c_void_p()
    assert _native.lib().afsk_live_create(4, 40, 18000, 14000, 96000, 8192, C.byref(h)) == _native.E_NO_DEVICE
    assert not h
    with pytest.raises(Exception, match="Invalid baud rate"):   # the reference's baud error comes first
        afskmodem.LiveReceiver(4, 41 * 2)
