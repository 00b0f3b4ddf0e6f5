"""Input sets of the transmit side's boundary sweeps (tests/test_gpu_tx_sweeps.py) and the placement conditions each
set was built for.  Not a test module.

Every sample writer lives in one translation unit (afsk_synth.hip with afsk_live_tx.hip and afsk_live_mix.hip).  The
batch modulator renders blocks of ``BLOCK`` samples and decides three things from where the tones end inside a block
(the silent-block shortcut, the TAIL instantiation, its dword masks); the live transmitter renders tiles of ``TILE``
samples in groups of 8 and has a slow path for the groups that hold a message's first or last tone samples.  The sets
here put those edges where a seed never would:

* ``ModSet`` (A1 ... A5): streams for ``batch.modulate_batch``.  ``reference`` renders them with the CPU oracle where
  ``bit_frames`` divides 48000 and with ``frames_ref`` -- the header's definition in plain numpy -- everywhere else.
* ``LiveSpec`` (B1 ... B6 and the hold form): one channel per placement.  Every channel queues a message X and then a
  message Y at position 0, a first ragged pull takes ``L`` samples of it, and the next pull is the one compared; ``L``
  puts a FEATURE (the first tone sample of Y, one past the last of X, Y's first data symbol, a coded bit of Y) at a
  chosen column of that pull.  ``realise`` runs the queue model (tests/live_tx_hold_model.py) and reads the columns that
  came out from the model's starts; ``check_live`` requires exactly the intended list.

Each set's ``check_*`` proves, from the reference side alone, that every intended placement happened:
tests/test_tx_sweep_inputs_host.py runs them on the CPU, the GPU sweeps run them again on the very sets they compare."""
import functools
import math
import os
import re
from dataclasses import dataclass, field

import numpy as np

from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests import live_mix_model as M
from tests import live_tx_hold_model as H

BLOCK = 16384                       # samples per block of modulate_kernel_t
TILE = 4096                         # samples per tile of live_tx_tile
MIN_BLOCKS = 8192                   # tiles from which a block of live_tx_tile renders two (x2) or four (x4) of them
TAIL = 4800
HI, LO = 32767, -32768
SENTINEL = 12345
MAX_BF = 1 << 20                    # the largest bit_frames the modulator renders (include/afsk_amd.h)
RATES = tuple(bf for bf in range(4, 48001, 4) if 48000 % bf == 0)     # what a Transmitter can have


def source_constants() -> dict:
    """The constants these sets rest on, read from the kernels' source."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "afskmodem_amd", "csrc")
    out = {}
    # a constant given as a number, and the sizes derived from them as the products their definitions spell out
    numbers = {"afsk_synth.hip": ("kModThreads", "kModIters", "kWinBytes"),
               "afsk_live_tx.hip": ("kTxThreads", "kTxIters", "kTxMinBlocks"),
               "afsk_live_mix.hip": ("kMixThreads", "kMixMaxDegree")}
    products = {"afsk_synth.hip": (("kModChunk", r"mod_chunk\(int iters, int threads = kModThreads\)\s*\{\s*return threads \* 8 "
                                                 r"\* iters;\s*\}", ("kModThreads", "kModIters")),),
                "afsk_live_tx.hip": (("kTxTile", r"constexpr\s+int\s+kTxTile\s*=\s*kTxThreads\s*\*\s*8\s*\*\s*kTxIters\s*;",
                                      ("kTxThreads", "kTxIters")),),
                "afsk_live_mix.hip": (("kMixTile", r"constexpr\s+int\s+kMixTile\s*=\s*kMixThreads\s*\*\s*8\s*;",
                                       ("kMixThreads",)),)}
    for fname, names in numbers.items():
        with open(os.path.join(csrc, fname)) as f:
            text = f.read()
        for name in names:
            m = re.findall(r"constexpr\s+(?:int|int32_t)\s+" + name + r"\s*=\s*(\d+)\s*;", text)
            assert len(m) == 1, (name, m)
            out[name] = int(m[0])
        for name, definition, factors in products[fname]:
            assert len(re.findall(definition, text)) == 1, name
            out[name] = 8 * math.prod(out[f] for f in factors)
        if fname == "afsk_synth.hip":                              # the launch that is built: kModIters stores per thread
            assert len(re.findall(r"return launch_modulate_t<kModIters>\(a, max_len, stream\);", text)) == 1
    return out


# ---------------------------------------------------------------------------------------------- the frame reference

def hamming74(nib: int) -> list:
    """p1 p2 d1 p3 d2 d3 d4 of a nibble d1 d2 d3 d4 (d1 its high bit)."""
    d1, d2, d3, d4 = (nib >> 3) & 1, (nib >> 2) & 1, (nib >> 1) & 1, nib & 1
    return [d1 ^ d2 ^ d4, d1 ^ d3 ^ d4, d1, d2 ^ d3 ^ d4, d2, d3, d4]


def symbol_kinds(payload: bytes, ts_cycles: int) -> np.ndarray:
    """1 = mark, 0 = space per symbol: the training cycles (mark, space), the terminator 1,0,0,0, then 14 Hamming bits
    per byte, the high nibble first."""
    bits = [1, 0] * max(int(ts_cycles), 0) + [1, 0, 0, 0]
    for b in bytes(payload):
        bits += hamming74(b >> 4) + hamming74(b & 15)
    return np.array(bits, np.uint8)


QUARTERS = np.array([[HI, HI, LO, LO], [HI, LO, HI, LO]], np.int16)     # space, mark over quarter symbols


def frames_ref(payload: bytes, bit_frames: int, ts_cycles: int, wav_quirk: bool, n: int | None = None) -> np.ndarray:
    """The header's definition of a modulated stream for ANY ``bit_frames`` that is a multiple of 4: every symbol's four
    quarter symbols of ``bit_frames / 4`` frames, 4800 zeros, and with the wav quirk ``out[m] = frames[m & ~1]``.  ``n``:
    truncate or zero pad to n samples (only the symbols that reach into them are rendered)."""
    assert bit_frames >= 4 and bit_frames % 4 == 0
    kinds = symbol_kinds(payload, ts_cycles)
    total = kinds.size * bit_frames + TAIL
    n = total if n is None else int(n)
    kinds = kinds[: -(-min(n, total) // bit_frames) + 1]
    frames = np.repeat(QUARTERS[kinds].reshape(-1), bit_frames // 4)
    frames = np.concatenate([frames, np.zeros(TAIL, np.int16)])
    if wav_quirk:
        frames = frames.copy()
        frames[1::2] = frames[0::2][: frames[1::2].size]
    out = np.zeros(n, np.int16)
    m = min(n, frames.size)
    out[:m] = frames[:m]
    return out


def tone_len(bf: int, ts: int, plen: int) -> int:
    return bf * (2 * max(ts, 0) + 4 + 14 * plen)


# ------------------------------------------------------------------------------------------- A. the batch modulator

@dataclass
class ModSet:
    payload: np.ndarray             # uint8 [n, stride]
    plen: np.ndarray                # int32 [n]
    bf: np.ndarray                  # int32 [n]
    ts: np.ndarray                  # int32 [n]
    off: np.ndarray                 # int64 [n]: streams alternate between odd and even sample offsets
    ln: np.ndarray                  # int32 [n]
    total: int                      # samples of the buffer: at least one untouched sample around every stream
    meta: list                      # [n] dicts: what the builder intended (never an expected value)

    @property
    def n(self):
        return int(self.bf.size)

    @property
    def lim(self):
        return self.bf.astype(np.int64) * (2 * self.ts.astype(np.int64) + 4 + 14 * self.plen.astype(np.int64))


def pack(streams) -> ModSet:
    """streams: dicts with bf, ts, payload (bytes), ln and whatever else describes the intent."""
    n = len(streams)
    stride = max(max(len(s["payload"]) for s in streams), 1)
    payload = np.zeros((n, stride), np.uint8)
    off = np.zeros(n, np.int64)
    at = 1
    for i, s in enumerate(streams):
        payload[i, : len(s["payload"])] = np.frombuffer(bytes(s["payload"]), np.uint8)
        at += (at & 1) == (i & 1)                                 # stream i begins at an odd offset when i is even
        off[i] = at
        at += int(s["ln"]) + 1
    i32 = lambda k: np.array([int(s[k]) for s in streams], np.int32)  # noqa: E731
    ms = ModSet(payload, np.array([len(s["payload"]) for s in streams], np.int32), i32("bf"), i32("ts"), off, i32("ln"),
                at + 8, [{k: v for k, v in s.items() if k != "payload"} for s in streams])
    assert (ms.off[1:] > ms.off[:-1] + ms.ln[:-1]).all() and set((ms.off % 2).tolist()) == {0, 1}
    return ms


def reference(ms: ModSet, wav_quirk: bool) -> np.ndarray:
    """int16 [total]: ``SENTINEL`` outside the streams, inside them the oracle's samples where bit_frames divides 48000,
    ``frames_ref`` at the other multiples of 4 up to 2^20, and zeros above (the header's rule)."""
    out = np.full(ms.total, SENTINEL, np.int16)
    divides = (48000 % ms.bf == 0)
    idx = np.nonzero(divides)[0]
    if idx.size:
        rel = np.zeros(idx.size, np.int64)
        rel[1:] = np.cumsum(ms.ln[idx][:-1].astype(np.int64))
        flat = O.modulate_batch(ms.payload[idx], ms.plen[idx], ms.bf[idx], ms.ts[idx], rel, ms.ln[idx],
                                int(ms.ln[idx].astype(np.int64).sum()), wav_quirk)
        for j, i in enumerate(idx):
            out[ms.off[i]: ms.off[i] + ms.ln[i]] = flat[rel[j]: rel[j] + ms.ln[i]]
    for i in np.nonzero(~divides)[0]:
        bf, ln = int(ms.bf[i]), int(ms.ln[i])
        row = np.zeros(ln, np.int16) if bf > MAX_BF else frames_ref(ms.payload[i, : ms.plen[i]].tobytes(), bf,
                                                                    int(ms.ts[i]), wav_quirk, ln)
        out[ms.off[i]: ms.off[i] + ln] = row
    return out


def seeded(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def set_a1() -> ModSet:
    """Every rate a Transmitter can have, two streams each: tones of about two and a half blocks (48 symbols where that
    is longer), one stream cut at the block multiple that holds the tones' end, one whole and zero padded."""
    streams = []
    for k, bf in enumerate(RATES):
        plen = 3
        n_sym = max(48, 2 * -(-(2 * BLOCK + BLOCK // 2) // (2 * bf)))
        ts = (n_sym - 4 - 14 * plen) // 2
        lim = tone_len(bf, ts, plen)
        for exact in (True, False):
            streams.append(dict(bf=bf, ts=ts, payload=seeded(1000 + k, plen), exact=exact,
                                ln=-(-lim // BLOCK) * BLOCK if exact else lim + TAIL + 37))
    return pack(streams)


def check_a1(ms: ModSet) -> None:
    assert sorted(set(ms.bf.tolist())) == list(RATES) and len(RATES) == 48
    assert (ms.ts >= 1).all() and (ms.plen >= 1).all() and (ms.lim > BLOCK).all()
    for bf in RATES:
        ln = ms.ln[ms.bf == bf]
        assert ln.size >= 2 and (ln % BLOCK == 0).any() and (ln % BLOCK != 0).any(), bf
    assert (ms.ln[ms.ln % BLOCK == 0] >= ms.lim[ms.ln % BLOCK == 0]).all()      # the block multiple holds the tones' end


A2_OFFSETS = {4: range(-16, 17), 12: range(-16, 17), 20: range(-16, 17), 28: range(-16, 17), 40: range(-16, 17),
              32: (0,), 160: (0,)}
A_BFS = tuple(A2_OFFSETS)
CUTS = range(-9, 10)


def geometry_for_tones(bf: int, lim: int):
    """(ts_cycles >= 1, payload_len >= 1) with bf * (2 ts + 4 + 14 plen) == lim."""
    assert lim % (2 * bf) == 0
    j = lim // (2 * bf)                                           # ts + 2 + 7 plen
    plen = min(20, (j - 3) // 7)
    ts = j - 2 - 7 * plen
    assert plen >= 1 and ts >= 1 and tone_len(bf, ts, plen) == lim, (bf, lim)
    return ts, plen


@functools.lru_cache(maxsize=None)
def set_a2() -> ModSet:
    """The tones' end ``lim`` at every reachable offset o from a block edge 16384 k, and for each a stream per
    stream_len in {lim + d, 16384 k + d}, d in -9 ... 9: the cut inside the last tone group, on it, in the silence."""
    streams = []
    for bf, offsets in A2_OFFSETS.items():
        for o in offsets:
            k = next((k for k in range(1, 2 * bf + 1) if (BLOCK * k + o) % (2 * bf) == 0), None)
            if k is None:
                continue
            lim = BLOCK * k + o
            ts, plen = geometry_for_tones(bf, lim)
            pay = seeded(2000 + bf * 100 + o, plen)
            for anchor, base in (("lim", lim), ("edge", BLOCK * k)):
                for d in CUTS:
                    streams.append(dict(bf=bf, ts=ts, payload=pay, ln=base + d, o=o, k=k, d=d, anchor=anchor))
    return pack(streams)


def reachable_tone_ends(bf: int, offsets) -> dict:
    """{o: smallest k} with lim - 16384 k == o for some message: lim runs over the multiples of 2 bf, so the offsets are
    the multiples of gcd(2 bf, 16384) and k <= 2 bf / gcd.  Found by walking the tone lengths, not the blocks."""
    g = math.gcd(2 * bf, BLOCK)
    want = [o for o in offsets if o % g == 0]
    found = {}
    for j in range(2, (2 * bf // g) * BLOCK // (2 * bf) + 64):
        lim = 2 * bf * j
        for o in want:
            if o not in found and lim - o >= BLOCK and (lim - o) % BLOCK == 0:
                found[o] = (lim - o) // BLOCK
    assert sorted(found) == want and max(found.values()) <= 2 * bf // g, (bf, found)
    return found


def check_a2(ms: ModSet) -> None:
    lim = ms.lim
    for bf, offsets in A2_OFFSETS.items():
        want = reachable_tone_ends(bf, offsets)
        rows = [i for i in range(ms.n) if ms.bf[i] == bf]
        got = {}
        for i in rows:
            m = ms.meta[i]
            assert lim[i] == BLOCK * m["k"] + m["o"], (bf, m)
            got.setdefault((m["o"], m["k"]), []).append(int(ms.ln[i]))
        assert sorted(got) == sorted(want.items()), (bf, sorted(got), want)
        for (o, k), lens in got.items():
            assert sorted(lens) == sorted([BLOCK * k + o + d for d in CUTS] + [BLOCK * k + d for d in CUTS]), (bf, o)
    assert (ms.ts >= 1).all() and (ms.plen >= 1).all()


A3_STEPS = (0, 2, -2, 4, -4)                                      # e in units of bit_frames


@functools.lru_cache(maxsize=None)
def set_a3() -> ModSet:
    """The first sample of the first data symbol at 16384 k + e, e in {0, +-2 bf, +-4 bf}: blocks that end one or two
    symbols before the data, and blocks that begin on it.  The data start bf * (2 ts + 4) is a multiple of 2 bf, so k is
    the smallest with 16384 k a multiple of 2 bf."""
    streams = []
    for bf in A_BFS:
        k = 2 * bf // math.gcd(2 * bf, BLOCK)
        for e in A3_STEPS:
            start = BLOCK * k + e * bf
            ts = start // (2 * bf) - 2
            streams.append(dict(bf=bf, ts=ts, payload=seeded(3000 + bf + e, 3), ln=tone_len(bf, ts, 3) + TAIL + 5, k=k,
                                e=e * bf))
    return pack(streams)


def check_a3(ms: ModSet) -> None:
    data0 = ms.bf.astype(np.int64) * (2 * ms.ts.astype(np.int64) + 4)
    for bf in A_BFS:
        sel = ms.bf == bf
        k = min(k for k in range(1, 2 * bf + 1) if (BLOCK * k) % (2 * bf) == 0)
        assert sorted((data0[sel] - BLOCK * k).tolist()) == sorted(e * bf for e in A3_STEPS), bf
    assert (ms.ts >= 1).all() and (ms.ln > ms.lim).all()


A4_BFS, A4_PLENS = (4, 8, 16, 40), (296, 512, 513, 1100)


@functools.lru_cache(maxsize=None)
def set_a4() -> ModSet:
    """Long payloads: the 256 byte values in order (every nibble pair), then seeded bytes."""
    streams = []
    for bf in A4_BFS:
        for plen in A4_PLENS:
            pay = bytes(range(256)) + seeded(4000 + bf + plen, plen - 256)
            streams.append(dict(bf=bf, ts=1, payload=pay, ln=tone_len(bf, 1, plen) + TAIL + 3))
    return pack(streams)


def check_a4(ms: ModSet) -> None:
    assert sorted(set(zip(ms.bf.tolist(), ms.plen.tolist()))) == sorted((b, p) for b in A4_BFS for p in A4_PLENS)
    for i in range(ms.n):
        assert ms.payload[i, :256].tolist() == list(range(256))
        bf, lim, data0 = int(ms.bf[i]), int(ms.lim[i]), 2 * int(ms.ts[i]) + 4
        blocks = range(1, -(-lim // BLOCK))
        assert len(blocks) >= 1
        # the byte of the first symbol of every block after the first: past byte 0, up to the payload's last
        first = [(BLOCK * b // bf - data0) // 14 for b in blocks]
        assert min(first) > 0 and max(first) <= int(ms.plen[i]) - 1, (i, first[:3])
    # the payloads reach past one block's span of bytes (bit_frames 4: 16384 / 56 = 292) and past one and two windows
    assert min(A4_PLENS) > BLOCK // (14 * min(A4_BFS)) and 512 in A4_PLENS and 513 in A4_PLENS and max(A4_PLENS) > 1024


A5_BFS = (36, 44, 52, 136, 1004, 2044, 4100, 65532, 1000000, 1048576)
A5_ABOVE = MAX_BF + 4


@functools.lru_cache(maxsize=None)
def set_a5() -> ModSet:
    """The rest of the C-ABI's domain: multiples of 4 that do not divide 48000, up to 2^20, and the first value above."""
    streams = []
    for bf in A5_BFS:
        for ts, plen in ((0, 0), (0, 1), (1, 0), (1, 1)) if bf < 1000000 else ((0, 1),):
            ln = tone_len(bf, ts, plen) + TAIL + 11 if bf < 1000000 else 6 * bf + 12345
            streams.append(dict(bf=bf, ts=ts, payload=bytes([0xA7][:plen]), ln=ln))
    streams.append(dict(bf=A5_ABOVE, ts=1, payload=b"\x5a", ln=20000))
    return pack(streams)


def check_a5(ms: ModSet) -> None:
    assert (48000 % ms.bf != 0).all() and (ms.bf % 4 == 0).all()
    assert sorted(set(ms.bf.tolist())) == sorted(A5_BFS + (A5_ABOVE,))
    for bf in A5_BFS[:-2]:
        assert sorted(zip(ms.ts[ms.bf == bf].tolist(), ms.plen[ms.bf == bf].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    big = ms.bf >= 1000000
    assert (ms.ln[big & (ms.bf <= MAX_BF)] > 6 * ms.bf[big & (ms.bf <= MAX_BF)]).all()      # two data symbols and more
    assert int(big.sum()) == 3 and MAX_BF in ms.bf.tolist() and A5_ABOVE == 1048580


MOD_SETS = {"a1": (set_a1, check_a1), "a2": (set_a2, check_a2), "a3": (set_a3, check_a3), "a4": (set_a4, check_a4),
            "a5": (set_a5, check_a5)}


# ------------------------------------------------------------------------------------------ B. the live transmitter

# q = bit_frames / 4 = 1, 2, 6, 7: the small-quarter tone code; 8: the first width of the large one; 10; 500.  28 divides
# 48000 in no baud rate: no Transmitter has it, the C entries take it (a multiple of 4 in 4 ... 48000), and its expected
# samples are ``frames_ref``'s -- which the host test holds against the oracle at every rate a Transmitter does have; 24
# is the widest small quarter that goes through ``Transmitter.wav_samples``.  (In this order the rated pairs, a
# geometry and the next one, put a small and a large quarter into one channel.)
LIVE_BFS = (4, 32, 8, 40, 24, 2000, 28)
LIVE_TS = {4: 3, 8: 2, 24: 1, 28: 1, 32: 1, 40: 1, 2000: 1, 48000: 0}
T2 = 2 * TILE + 17                      # the compared pull: three tiles, the last one partial
T4 = 5 * TILE + 17                      # ... of the four-tiles-per-block objects: a row is more than one block
EDGES = (0, TILE, 2 * TILE)
MAXP, DEPTH = 512, 2                    # (the X of a T4 set at bit_frames 4 holds 367 bytes)
B3_COLS = (100, TILE + 37, 2 * TILE - 4)
B5_BYTES = (0, 1, 200)


def training_time(bf: int, ts: int) -> float:
    """A training time that gives ``Transmitter(48000 / bf, t).ts_cycles == ts`` (int(baud * t / 2), ref:438); 0 for 0."""
    return 0.0 if ts == 0 else (2 * ts + 0.5) * bf / 48000.0


@dataclass
class Chan:
    ex: int                         # table entry (geometry) of X
    ey: int                         # ... of Y
    px: bytes
    py: bytes
    feature: str                    # "Y0", "X1", "data", "bit"
    bit: int                        # the coded bit of Y ("bit")
    col: int                        # the column of the compared pull the feature is to fall on
    len2: int | None = None         # the compared pull's own length for this channel (None: the whole pull)


@dataclass
class LiveSpec:
    name: str
    kind: str                       # "uniform", "mixed", "rated"
    table: list                     # [(bit_frames, ts_cycles)]
    chans: list
    T: int
    L: np.ndarray = field(default=None)      # int64 [n]: samples of the first, ragged pull

    @property
    def n(self):
        return len(self.chans)


def b4_offsets(bf: int) -> list:
    return [-2 * bf, -bf - 1, -bf, -bf + 1, -1, 0, 1, bf - 1, bf, bf + 1, 2 * bf]


def intent(name: str, bf: int, T: int = T2) -> list:
    """The placements of a set as (feature, coded bit, column, the compared pull's length or None); ``bf``: of the
    message that carries the feature."""
    edges = EDGES + ((4 * TILE,) if T == T4 else ())               # (T4: also the edge between the row's two blocks)
    if name in ("b1", "b2"):
        return [("Y0" if name == "b1" else "X1", 0, E + d, None) for E in edges for d in range(-17, 18) if E + d >= 0]
    if name == "b3":
        return [(f, 0, col, col + d) for f in ("Y0", "X1") for col in B3_COLS for d in CUTS]
    if name == "b4":
        return [("data", 0, TILE + d, None) for d in b4_offsets(bf)]
    if name == "b5":
        return [("bit", 14 * byte + i, TILE + d, None) for byte in B5_BYTES for i in range(14) for d in (-1, 0, 1)]
    if name == "b6":
        return [("Y0", 0, TILE + d, None) for d in range(-24, 9)]
    raise KeyError(name)


PY_LEN = {"b1": 2, "b2": 2, "b3": 2, "b4": 3, "b5": 256, "b6": 0}


def filler_len(bf: int, ts: int, T: int) -> int:
    """Payload bytes of an X whose tones are longer than the compared pull: any column can be its end."""
    return max(1, -(-(-(-(T + 64) // bf) - 2 * ts - 4) // 14))


def live_spec(name: str, kind: str, bfs=LIVE_BFS, T: int = T2) -> LiveSpec:
    """One channel per placement and geometry: ``uniform`` -- one bit_frames --, ``mixed`` -- every geometry of ``bfs``,
    X and Y of a channel at the channel's --, ``rated`` -- X and Y at different rates: for every geometry g and the next
    one h in ``bfs`` (cyclic) the channels (X at h, Y at g) and (X at g, Y at h)."""
    ts_of = {bf: 0 for bf in bfs} if name == "b6" else LIVE_TS
    table = [(bf, ts_of[bf]) for bf in bfs]
    k = len(table)
    if kind == "uniform":
        assert k == 1
    pairs = {"uniform": [(0, 0)], "mixed": [(e, e) for e in range(k)],
             "rated": [p for e in range(k) for p in (((e + 1) % k, e), (e, (e + 1) % k))]}[kind]
    chans = []
    for ex, ey in pairs:
        (bfx, tsx), (bfy, _) = table[ex], table[ey]
        for feature, bit, col, len2 in intent(name, bfx if feature_in_x(name) else bfy, T):
            c = len(chans)
            px = b"" if name == "b6" else seeded(5000 + c, filler_len(bfx, tsx, T))
            py = (bytes(range(256)) if name == "b5" else seeded(6000 + c, PY_LEN[name]))
            chans.append(Chan(ex, ey, px, py, feature, bit, col, len2))
    spec = LiveSpec(name, kind, table, chans, T)
    spec.L = np.array([feature_pos(spec, ch) - ch.col for ch in chans], np.int64)
    assert (spec.L >= 0).all()
    return spec


def feature_in_x(name: str) -> bool:
    return name == "b2"


def feature_pos(spec: LiveSpec, ch: Chan) -> int:
    """Where the builder expects the feature in the channel's stream (X starts at 0, Y follows its silent tail)."""
    (bfx, tsx), (bfy, tsy) = spec.table[ch.ex], spec.table[ch.ey]
    x1 = tone_len(bfx, tsx, len(ch.px))
    y0 = x1 + TAIL
    return {"X1": x1, "Y0": y0, "data": y0 + bfy * (2 * tsy + 4), "bit": y0 + bfy * (2 * tsy + 4 + ch.bit)}[ch.feature]


def submit_lists(spec: LiveSpec, n: int | None = None):
    """(channels, payloads, table entries) of the submit that queues X then Y on every channel; ``n`` channels: channel
    c carries placement c mod P."""
    n = spec.n if n is None else n
    chans, pays, entries = [], [], []
    for c in range(n):
        ch = spec.chans[c % spec.n]
        chans += [c, c]
        pays += [ch.px, ch.py]
        entries += [ch.ex, ch.ey]
    return chans, pays, entries


def realise(spec: LiveSpec, wav=None):
    """The queue model after the submit and the first, ragged pull, and the column of the compared pull every channel's
    feature fell on -- read from the MODEL's starts and sample counts, not from ``feature_pos`` --, and the model's
    (start, n_samples) of the 2 n messages and pending after the first pull."""
    model = H.HoldTxRatedModel(spec.n, spec.table, DEPTH, MAXP, wav=wav)
    status, start, ns = model.submit(*submit_lists(spec))
    assert (status == _native.LIVE_TX_QUEUED).all()
    pend = model.pull_ragged(int(spec.L.max()), spec.L.tolist())
    cols = []
    for c, ch in enumerate(spec.chans):
        bfy, tsy = spec.table[ch.ey]
        x0, nx, y0 = int(start[2 * c]), int(ns[2 * c]), int(start[2 * c + 1])
        at = {"X1": x0 + nx - TAIL, "Y0": y0, "data": y0 + bfy * (2 * tsy + 4),
              "bit": y0 + bfy * (2 * tsy + 4 + ch.bit)}[ch.feature]
        cols.append(at - model.pos[c])
    return model, np.array(cols, np.int64), (start, ns, pend)


def lens2(spec: LiveSpec, form: str):
    """The compared pull's lengths: the set's own (B3), else None for the plain form and, for the ragged one, the whole
    pull on even channels and up to 22 samples less on odd ones."""
    if spec.name == "b3":
        return [ch.len2 for ch in spec.chans]
    if form != "ragged":
        return None
    return [spec.T - (c % 23 if c & 1 else 0) for c in range(spec.n)]


def check_live(spec: LiveSpec, cols) -> None:
    """Per geometry pair, the realised (feature, bit, column, length) are exactly the set's intended list -- written out
    here again, not taken from the builder's channels."""
    k = len(spec.table)
    groups = {}
    for ch, col in zip(spec.chans, cols.tolist()):
        groups.setdefault((ch.ex, ch.ey), []).append((ch.feature, ch.bit, col, ch.len2))
    want_pairs = {"uniform": [(0, 0)], "mixed": [(e, e) for e in range(k)],
                  "rated": [((e + 1) % k, e) for e in range(k)] + [(e, (e + 1) % k) for e in range(k)]}[spec.kind]
    assert sorted(groups) == sorted(want_pairs)
    for (ex, ey), got in groups.items():
        bf = spec.table[ex if spec.name == "b2" else ey][0]
        edges = EDGES + ((4 * TILE,) if spec.T == T4 else ())
        if spec.name in ("b1", "b2"):
            want = [("Y0" if spec.name == "b1" else "X1", 0, E + d, None) for E in edges for d in range(-17, 18)]
            want = [w for w in want if w[2] >= 0]
            assert len(want) == 35 * len(edges) - 17
        elif spec.name == "b3":
            want = [(f, 0, col, col + d) for f in ("Y0", "X1") for col in B3_COLS for d in range(-9, 10)]
        elif spec.name == "b4":
            want = [("data", 0, TILE + d, None)
                    for d in (-2 * bf, -bf - 1, -bf, -bf + 1, -1, 0, 1, bf - 1, bf, bf + 1, 2 * bf)]
            assert len(set(want)) == 11
        elif spec.name == "b5":
            want = [("bit", b, TILE + d, None) for b in list(range(28)) + list(range(2800, 2814)) for d in (-1, 0, 1)]
        else:
            want = [("Y0", 0, TILE + d, None) for d in range(-24, 9)]
        assert sorted(got, key=str) == sorted(want, key=str), (spec.name, spec.kind, ex, ey)
    if spec.name == "b6":
        assert all(ts == 0 for _, ts in spec.table) and all(ch.px == b"" and ch.py == b"" for ch in spec.chans)
    if spec.kind == "rated":
        assert all(spec.table[ch.ex][0] != spec.table[ch.ey][0] for ch in spec.chans)


def check_rows(spec: LiveSpec, model, cols, exp) -> None:
    """The same from the expected samples ``exp`` (the model's ``expected(T)``): silence on one side of a message's
    first or last tone sample, a rail value on the other."""
    T = exp.shape[1]
    for c, (ch, col) in enumerate(zip(spec.chans, cols.tolist())):
        assert 0 <= col <= T                                      # (column T: the feature is the next pull's first sample)
        if ch.feature == "Y0":
            assert (col == T or exp[c, col] in (HI, LO)) and (col == 0 or exp[c, col - 1] == 0), (c, col)
        elif ch.feature == "X1":
            assert (col == T or exp[c, col] == 0) and (col == 0 or exp[c, col - 1] in (HI, LO)), (c, col)
        else:
            assert exp[c, col] in (HI, LO) and exp[c, col - 1] in (HI, LO), (c, col)


HOLD_OFFSETS = range(-9, 10)
HOLD_FIRST = 8                          # samples of the held pull


def hold_case(table, d: int, wav=None):
    """The hold form of B1: one message per channel (channel c at table entry c) on idle channels, a pull of
    ``HOLD_FIRST`` samples with every channel held and holdoff = 4096 + d -- the deferred message then starts at that
    column of the next pull.  Returns the model before the two pulls and the payloads."""
    model = H.HoldTxRatedModel(len(table), table, DEPTH, MAXP, wav=wav)
    pays = [seeded(7000 + 32 * e + d, 2) for e in range(len(table))]
    model.submit(list(range(len(table))), pays, list(range(len(table))))
    return model, pays


TILES_N = 5462                          # channels from which T2's three tiles share a block by twos, T4's six by fours


class WavCache:
    """``Transmitter(48000 / bf, training_time(bf, ts)).wav_samples(payload)`` -- the host mirror the golden digests pin
    to the reference -- kept per (geometry, payload); ``of(table)`` is the ``wav(payload, entry)`` the queue models take."""

    def __init__(self):
        self.tr, self.wavs = {}, {}

    def wav(self, geom, payload):
        key = (geom, bytes(payload))
        if key not in self.wavs:
            bf, ts = geom
            if 48000 % bf:                                        # no Transmitter: the header's definition
                self.wavs[key] = frames_ref(bytes(payload), bf, ts, True)
                return self.wavs[key]
            if geom not in self.tr:
                import afskmodem_amd as afskmodem
                self.tr[geom] = afskmodem.Transmitter(48000 // bf, training_time(bf, ts))
                assert self.tr[geom].ts_cycles == ts and self.tr[geom].bit_frames == bf
            self.wavs[key] = self.tr[geom].wav_samples(bytes(payload))
        return self.wavs[key]

    def of(self, table):
        table = [tuple(g) for g in table]
        return lambda payload, entry: self.wav(table[entry], payload)


# ------------------------------------------------------------------------------------------------------- C. noise

NOISE_SEED = 4711
NOISE_BASES = (0, 1, (1 << 32) - 1)     # stream_idx_base: from the second stream on, the last one wraps
NOISE_SCALES = (0, 1, 1 << 24, (1 << 31) - 1)


@dataclass
class NoiseSet:
    clean: np.ndarray               # int16 [total]: the streams, SENTINEL between them
    off: np.ndarray                 # int64 [n], all odd
    ln: np.ndarray                  # int32 [n]
    scale: np.ndarray               # int32 [n]
    rail: list                      # [n] bool: rail-valued samples (else random ones)
    total: int


@functools.lru_cache(maxsize=None)
def noise_set() -> NoiseSet:
    """Streams of 1 ... 17 and 2048 k +- d samples (noise_kernel's partial tail at every length of it, either side of
    its 2048-sample block) at odd offsets, each with every scale on rail-valued and on random samples."""
    rng = np.random.default_rng(8)
    lens = list(range(1, 18)) + [2048 * k + d for k in (1, 2) for d in range(-9, 10)]
    off, ln, scale, rail, parts, at = [], [], [], [], [], 1
    for n in lens:
        for s in NOISE_SCALES:
            for r in (False, True):
                x = rng.choice(np.array([HI, LO], np.int16), n) if r else rng.integers(-32768, 32768, n, dtype=np.int16)
                gap = 1 + ((at + n + 1) % 2 == 0)                 # the next stream begins at an odd offset too
                off.append(at), ln.append(n), scale.append(s), rail.append(r)
                parts += [x, np.full(gap, SENTINEL, np.int16)]
                at += n + gap
    clean = np.concatenate([np.full(1, SENTINEL, np.int16)] + parts + [np.full(8, SENTINEL, np.int16)])
    return NoiseSet(clean, np.array(off, np.int64), np.array(ln, np.int32), np.array(scale, np.int32), rail, clean.size)


def noise_reference(ns: NoiseSet, base: int) -> np.ndarray:
    """The oracle's generator on every stream; where the stream index base + s wraps past 2^32, the numpy restatement of
    the header's formula (tests/live_mix_model.py: the oracle takes the index as it is given, the kernel adds in uint32)."""
    out = ns.clean.copy()
    for s in range(ns.off.size):
        row = ns.clean[ns.off[s]: ns.off[s] + ns.ln[s]]
        idx = base + s
        got = O.add_noise(row, NOISE_SEED, idx, int(ns.scale[s])) if idx < (1 << 32) else \
            M.noise_direct(row, NOISE_SEED, idx & 0xFFFFFFFF, int(ns.scale[s]), 0)
        out[ns.off[s]: ns.off[s] + ns.ln[s]] = got
    return out
