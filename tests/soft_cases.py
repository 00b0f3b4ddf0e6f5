"""Shared by tests/test_soft_cases_host.py and tests/test_gpu_soft_large.py: the prototype streams whose soft
outputs the CPU oracle computes once per rate, their tiling up to the stream counts that arm the large-launch kernel
forms, output buffers with sentinel guards around them, and the checker of a launch's write footprint.  Not a
conftest, not a test module.

The oracle's soft pass (``demod_batch_soft``) is a Python loop over streams, so no large launch is ever sent to it
whole: it runs over ``prototypes(bf)`` -- about fifty distinct short streams per rate -- and a launch of n streams
is those prototypes repeated and shuffled with a seed.  Every copy must equal its prototype's oracle row."""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

import afskmodem_amd as afskmodem
from afskmodem_amd import _native, batch, synth
from oracle import afsk_oracle as O
from tests.gpu_common import LARGE_LAUNCH_BAUDS, large_launch_streams

# the 30 rates of test_large_launch_arms_l2_warming_on_every_path, then the six other rates a Receiver can have:
# together the 36 compile-time geometries (AFSK_FAST_BF_LIST + AFSK_GP_BF_LIST)
MIXED_BAUDS = LARGE_LAUNCH_BAUDS + (150, 100, 375, 250, 240, 160, 120, 96, 80, 75, 48, 32, 24)
ALL_BAUDS = MIXED_BAUDS + (125, 60, 50, 40, 30, 25)
RT_BIT_FRAMES = (136, 1004)                 # run-time geometries: no divisor of 48000 (C-ABI only)
MIXED_BIT_FRAMES = tuple(48000 // b for b in MIXED_BAUDS) + RT_BIT_FRAMES
ALL_BIT_FRAMES = tuple(48000 // b for b in ALL_BAUDS) + RT_BIT_FRAMES
# one rate per round-loop family, for the launches that arm the hint without the warming
HINT_ONLY_BIT_FRAMES = (40, 20, 160, 16, 48, 100, 320, 128, 1000, 136)

# stream counts of the GPU cases; tests/test_soft_cases_host.py ties each to the thresholds in afsk_demod_ring.h
N_MIXED = (6200, 8256)                      # hint alone / hint and warming (per-stream entry)
N_GROUPED = (4200, 8256)                    # armed for the grouped walk and not for the mixed one / both
N_UNIFORM = 8256                            # every uniform kernel's large form, hint and warming
N_UNIFORM_BF8 = 16500                       # bit_frames 8 arms later
N_HINT_ONLY = 4200                          # uniform kernels: hint without warming
N_SMALL_MAX = 400                           # the small-launch forms: the prototypes once, no tiling

OUT_STRIDE = 96                             # holds the longest prototype payload (80 bytes)
NARROW_OUT_STRIDE, NARROW_MARGIN_STRIDE = 5, 37      # both truncate, both odd, no multiple of a lane count
PROTO_CAP = 48000                           # samples of a base prototype at most
FLUSH_PAYLOAD = 80                          # > 64: the receiver writes one 64-byte batch mid-stream
FLUSH_MAX_BIT_FRAMES = 20

BYTE_SENTINEL = 0xA5
INT_SENTINEL = -0x5A5A5A5B                  # the same bit pattern in an int32
MARGIN_SENTINEL = -2 ** 31 + 12345          # no margin: |space_diff - mark_diff| <= 65535
INT_FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")
REFUSED_LENGTHS = (0, 4095, -1)             # too short, too short by one sample, a device-side length out of range
REFUSED_BIT_FRAMES = (42, 0)                # no multiple of 4 / not positive: per-stream and grouped entries only


def oracle_threads() -> int:
    return min(16, os.cpu_count() or 1)


def source_thresholds() -> dict:
    """The stream counts from which afsk_demod_ring.h arms the large-launch measures, read from the source."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "afskmodem_amd", "csrc",
                        "afsk_demod_ring.h")
    with open(path) as f:
        text = f.read()
    out = {}
    for name in ("kHintMinStreams", "kHintMinStreamsGrouped", "kHintMinStreamsUniform", "kHintMinStreamsShort4",
                 "kHintMinStreamsShort8", "kWarmMinStreams"):
        m = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


# ------------------------------------------------------------------------------------------------ prototypes
@dataclass(frozen=True)
class ProtoSet:
    """Distinct streams of one or several rates with the oracle's rows for them.  ``streams[i]`` is zero padded to a
    multiple of 8 samples (a stream of a launch starts on 16 bytes), ``lens[i]`` is its true length."""
    streams: tuple
    lens: np.ndarray            # int32 [P]
    bf: np.ndarray              # int32 [P]
    want: dict                  # oracle rows: INT_FIELDS, corrected, n_symbols [P]; bytes [P, OUT_STRIDE]; margins [P, W]
    forced: np.ndarray          # indices of the forced-correction prototypes

    @property
    def margin_stride(self) -> int:
        """Wide enough for every symbol of every prototype (the largest K + 8, or a little more)."""
        return int(self.want["margins"].shape[1])


def symbols_in(lens, ci, bf):
    """K: the symbols a stream of ``lens`` samples holds behind clock index ``ci`` (sample ci + k * bf with a whole
    symbol and one more sample behind it: the reference's i < len - bf); 0 for a refused stream."""
    lens, ci, bf = (np.asarray(a, np.int64) for a in (lens, ci, bf))
    return np.where(ci >= 0, (lens - ci - 1) // np.maximum(bf, 1), 0)


def _forced_correction_streams(clean, bf, term_frame, n_codewords, mark, space):
    """``clean`` with data symbol 7 * cw + cw % 7 of every third codeword replaced by the opposite tone (each
    position of a codeword is hit in turn), behind leads of 0, 7 and 12 samples."""
    y = clean.copy()
    for cw in range(0, n_codewords, 3):
        p = term_frame + (7 * cw + cw % 7) * bf
        was_mark = np.array_equal(y[p: p + bf], mark)
        assert was_mark or np.array_equal(y[p: p + bf], space), (bf, cw)
        y[p: p + bf] = space if was_mark else mark
    return [np.concatenate([np.zeros(lead, np.int16), y]) for lead in (0, 7, 12)]


def _frames_rt(bf, data, ts):
    """Transmitter.frames for a bit_frames no Transmitter can have (a multiple of 4 that does not divide 48000), with
    the tones of the kernels' run-time geometry: a space is one square period per symbol, a mark two.  Returns the
    frames, the mark and the space tone."""
    hi, lo = (int(v) for v in O.space_tone(1200)[[0, -1]])
    space = np.repeat(np.array([hi, lo], np.int16), bf // 2)
    mark = np.tile(np.repeat(np.array([hi, lo], np.int16), bf // 4), 2)
    ecc = O.ecc_encode("".join(format(b, "08b") for b in data))
    parts = [mark, space] * ts + [mark, space, space, space] + [mark if b == "1" else space for b in ecc]
    return np.concatenate(parts + [np.zeros(4800, np.int16)]), mark, space


def _base_streams_rt(bf, n=48):
    """The base set of a run-time geometry, after test_uniform_runtime_geometry_large_launch (two payload bytes
    behind a short training sequence, every seventh without the tail silence, every third noisy); odd leads give
    both parities of the clock index."""
    total = 12000 if bf < 512 else 44000
    rng = np.random.default_rng(bf)
    payload = synth.payload_bytes(bf, 0, n, 2)
    out = []
    for i in range(n):
        x = _frames_rt(bf, payload[i].tobytes(), max(2, 3000 // bf))[0]
        ln = total - (4800 + (i // 7) % 5 if i % 7 == 0 else 0)
        x = x[:ln] if ln <= len(x) else np.concatenate([x, np.zeros(ln - len(x), np.int16)])
        x = O.add_noise(x, bf, i, synth.snr_to_scale_q24(8.0 if i % 3 == 0 else 40.0))
        lead = int(rng.integers(0, 40)) if i % 3 else 0
        out.append(np.concatenate([np.zeros(lead, np.int16), x]))
    return out


def _oracle_rows(streams, bf):
    lens = np.array([len(x) for x in streams], np.int32)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)]).astype(np.int64)
    flat = np.concatenate(streams)
    bfa = np.full(len(streams), bf, np.int32)
    width = int((lens.astype(np.int64) - 1).max() // bf) + 8            # K <= (len - 1) // bf
    want = O.demod_batch_soft(flat, off, lens, bfa, 14000, out_stride=OUT_STRIDE, margin_stride=width)
    return lens, want


def prototypes(bf: int, base: int = 48) -> ProtoSet:
    """The prototype set of one rate: ``base`` streams of the base set (large_launch_streams: odd leads, weak
    signals, late starts, two bursts with a gap, noise; capped at PROTO_CAP samples), three with forced corrections
    (uncapped: ten codewords take 150,000 samples at 24 baud) and for bit_frames <= 20 one whose payload is flushed
    mid-stream.  Cached: the arrays are read-only."""
    return _prototypes(int(bf), int(base))


@functools.lru_cache(maxsize=None)
def _prototypes(bf: int, base: int) -> ProtoSet:
    rng = np.random.default_rng(5000 + bf)
    data = rng.integers(0, 256, 5, dtype=np.uint8).tobytes()           # 10 codewords: 0, 3, 6 and 9 are hit
    if 48000 % bf == 0:
        baud = 48000 // bf
        flat, off, ln, _ = large_launch_streams(48, (baud,), 1000 + baud)
        streams = [flat[o: o + min(int(l), PROTO_CAP)] for o, l in zip(off, ln)][:base]
        clean = afskmodem.Transmitter(baud, 0.08).frames(data)
        mark, space = O.mark_tone(baud), O.space_tone(baud)
    else:
        streams = _base_streams_rt(bf)[:base]
        clean, mark, space = _frames_rt(bf, data, max(2, 3000 // bf))
    term = int(O.demod_batch(clean, [0], [len(clean)], [bf], 14000, out_stride=OUT_STRIDE)["term_frame"][0])
    forced = np.arange(len(streams), len(streams) + 3)
    streams = streams + _forced_correction_streams(clean, bf, term, 2 * len(data), mark, space)
    if bf <= FLUSH_MAX_BIT_FRAMES:
        streams.append(afskmodem.Transmitter(48000 // bf, 0.08).frames(
            rng.integers(0, 256, FLUSH_PAYLOAD, dtype=np.uint8).tobytes()))
    lens, want = _oracle_rows(streams, bf)
    padded = []
    for x in streams:
        p = np.concatenate([x, np.zeros((-len(x)) % 8, np.int16)])
        p.setflags(write=False)
        padded.append(p)
    for a in want.values():
        a.setflags(write=False)
    return ProtoSet(tuple(padded), lens, np.full(len(streams), bf, np.int32), want, forced)


def merged(bit_frames, base: int = 48) -> ProtoSet:
    """The prototype sets of several rates as one (margin rows zero padded to the widest)."""
    sets = [prototypes(int(b), base) for b in bit_frames]
    if len(sets) == 1:
        return sets[0]
    width = max(s.margin_stride for s in sets)
    want = {k: np.concatenate([s.want[k] for s in sets]) for k in sets[0].want if k != "margins"}
    want["margins"] = np.concatenate([np.pad(s.want["margins"], ((0, 0), (0, width - s.margin_stride))) for s in sets])
    first = np.cumsum([0] + [len(s.streams) for s in sets[:-1]])
    return ProtoSet(tuple(x for s in sets for x in s.streams), np.concatenate([s.lens for s in sets]),
                    np.concatenate([s.bf for s in sets]), want,
                    np.concatenate([s.forced + f for s, f in zip(sets, first)]))


def assert_conditions(ps: ProtoSet, mixed: bool = False) -> None:
    """What a case relies on, asserted on the ORACLE's rows before anything is launched."""
    w = ps.want
    for bf in np.unique(ps.bf):
        sel = ps.bf == bf
        ci = w["clock_idx"][sel]
        assert (ci[ci >= 0] & 1).any() and not (ci[ci >= 0] & 1).all(), f"bit_frames {bf}: one parity of clock_idx only"
        assert int((w["corrected"][sel] > 0).sum()) >= 3, f"bit_frames {bf}: fewer than 3 prototypes with corrections"
        if bf <= FLUSH_MAX_BIT_FRAMES:
            assert int(w["nbytes"][sel].max()) >= FLUSH_PAYLOAD, f"bit_frames {bf}: no mid-stream flush"
    assert (w["corrected"][ps.forced] > 0).all()
    if mixed:
        ci = w["clock_idx"]
        assert len({(2 * int(c)) & 15 for c in ci[ci >= 0]}) == 8, "a ring shift is missing"


# ------------------------------------------------------------------------------------------------ launches
@dataclass
class Launch:
    flat: np.ndarray            # int16: every stream of the launch
    off: np.ndarray             # int64 [n]
    lens: np.ndarray            # int32 [n] what the DEVICE is told (refused values included)
    host_lens: np.ndarray       # int32 [n] the true lengths (what a host-side plan is built from)
    bf: np.ndarray              # int32 [n] refused values included
    want: dict                  # the model: the prototype's oracle row, the refusal row for a refused stream
    refused: np.ndarray         # bool [n]
    margin_stride: int          # the wide one


def refuse(launch: Launch, slots, kinds) -> Launch:
    """``launch`` with the streams ``slots`` refused, kind after kind in turn: an int is a length the device is
    told, ("bf", v) an invalid bit_frames.  The model row of a refused stream is the oracle's: status, 0 bytes,
    0 bits, clock index -1, terminator -1, 0 corrected, no margin."""
    slots = np.asarray(slots)
    lens, bf = launch.lens.copy(), launch.bf.copy()
    want = {k: v.copy() for k, v in launch.want.items()}
    status = np.zeros(slots.size, np.int32)
    for j, kind in enumerate(kinds):
        sel = slots[j::len(kinds)]
        if isinstance(kind, tuple):
            bf[sel] = kind[1]
            status[j::len(kinds)] = _native.ST_INVALID_BAUD
        else:
            lens[sel] = kind
            status[j::len(kinds)] = _native.ST_BAD_LENGTH if kind < 0 else _native.ST_TOO_SHORT
    for f, v in (("nbytes", 0), ("nbits", 0), ("clock_idx", -1), ("term_frame", -1), ("corrected", 0), ("n_symbols", 0)):
        want[f][slots] = v
    want["status"][slots] = status
    want["bytes"][slots] = 0
    want["margins"][slots] = 0
    refused = launch.refused.copy()
    refused[slots] = True
    return Launch(launch.flat, launch.off, lens, launch.host_lens, bf, want, refused, launch.margin_stride)


def build_launch(ps: ProtoSet, n: int | None, seed: int, invalid_bf: bool = False, refused_every: int = 9) -> Launch:
    """``n`` streams: the prototypes repeated and shuffled (None: each once, in order), about one in
    ``refused_every`` refused -- between decoded ones -- by length, with ``invalid_bf`` also by bit_frames."""
    P = len(ps.streams)
    if n is None:
        order = np.arange(P)
    else:
        order = np.tile(np.arange(P), -(-n // P))[:n]
        np.random.default_rng(seed).shuffle(order)         # neighbours in a workgroup differ in rate and length
    n = order.size
    padded = np.array([len(x) for x in ps.streams], np.int64)[order]
    off = np.concatenate([[0], np.cumsum(padded[:-1])]).astype(np.int64)
    flat = np.concatenate([ps.streams[i] for i in order])                  # one copy of every slot's samples
    want = {k: v[order] for k, v in ps.want.items()}
    lens = ps.lens[order].copy()
    launch = Launch(flat, off, lens, lens.copy(), ps.bf[order].copy(), want, np.zeros(n, bool), ps.margin_stride)
    if not refused_every:
        return launch
    kinds = REFUSED_LENGTHS + (tuple(("bf", v) for v in REFUSED_BIT_FRAMES) if invalid_bf else ())
    return refuse(launch, np.arange(refused_every // 2, n, refused_every), kinds)


# ------------------------------------------------------------------------------------------------ guarded outputs
@dataclass
class Guards:
    """The whole allocations whose interiors a guarded DemodResult views."""
    bytes: "object"             # uint8 [n + 2, stride]
    ints: dict                  # INT_FIELDS + corrected -> int32 [n + 16]
    margins: "object"           # int32 [n + 2, margin_stride]


def guarded_result(n: int, out_stride: int, margin_stride: int, device) -> batch.DemodResult:
    """A DemodResult for ``out=`` whose tensors are interior views of larger allocations prefilled with sentinels
    (``result.guards``): bytes rows [1, n + 1) of n + 2, each int32 array elements [8, n + 8) of n + 16, margins rows
    [1, n + 1) of n + 2."""
    import torch
    g = Guards(torch.full((n + 2, out_stride), BYTE_SENTINEL, dtype=torch.uint8, device=device),
               {f: torch.full((n + 16,), INT_SENTINEL, dtype=torch.int32, device=device)
                for f in INT_FIELDS + ("corrected",)},
               torch.full((n + 2, margin_stride), MARGIN_SENTINEL, dtype=torch.int32, device=device))
    res = batch.DemodResult(g.bytes[1: n + 1], *(g.ints[f][8: n + 8] for f in INT_FIELDS),
                            corrected=g.ints["corrected"][8: n + 8], margins=g.margins[1: n + 1])
    res.guards = g  # type: ignore[attr-defined]
    return res


def _first(mask):
    idx = np.argwhere(mask)
    return idx[:5].tolist()


def check_footprint(result, guards: Guards, want: dict, lens, bf, one_wave: bool = True, tag: str = "") -> None:
    """Zero tolerance: ``result`` (a guarded DemodResult after a launch) holds the model ``want`` and nothing else
    was written.  ``lens`` / ``bf``: what the launch was given per stream.
     F1  byte row s: [0, min(nbytes, stride)) is the model's, the rest of the row and both guard rows are untouched;
     F2  nbytes, nbits, clock_idx, term_frame, status are the model's for every stream, the guards untouched;
     F3  corrected likewise (0 for a refused stream);
     F4  margin row s: [0, min(n_symbols, stride)) is the model's; a refused stream's row and the guard rows are
         untouched; with ``one_wave`` every entry at or beyond K = (len - clock_idx - 1) // bf is untouched too (no
         symbol exists there).  [n_symbols, min(K, stride)) is unspecified and not looked at; the split path's
         segments (``one_wave`` False) may fill their own row."""
    del result                                             # its tensors are views of the guards
    n = int(want["status"].shape[0])
    gb = guards.bytes.cpu().numpy()
    stride = gb.shape[1]
    assert gb.shape[0] == n + 2
    refused = want["clock_idx"] < 0
    # F2, F3
    for f in INT_FIELDS + ("corrected",):
        a = guards.ints[f].cpu().numpy()
        assert (a[:8] == INT_SENTINEL).all() and (a[n + 8:] == INT_SENTINEL).all(), f"{tag} {f}: guard overwritten"
        bad = np.nonzero(a[8: n + 8] != want[f])[0]
        assert bad.size == 0, (f"{tag} {f}: {bad.size} streams differ, first {bad[:5]}: got {a[8 + bad[:5]]} "
                               f"want {want[f][bad[:5]]} (refused: {refused[bad[:5]]})")
    # F1
    assert (gb[0] == BYTE_SENTINEL).all() and (gb[n + 1] == BYTE_SENTINEL).all(), f"{tag} bytes: guard row overwritten"
    rows = gb[1: n + 1]
    col = np.arange(stride)[None, :]
    inside = col < np.minimum(want["nbytes"], stride)[:, None]
    w = min(stride, want["bytes"].shape[1])
    assert not inside[:, w:].any(), f"{tag}: the model's byte rows are narrower than a payload"
    model = np.full(rows.shape, BYTE_SENTINEL, np.uint8)
    model[:, :w] = np.where(inside[:, :w], want["bytes"][:, :w], BYTE_SENTINEL)
    bad = rows != model
    assert not bad.any(), f"{tag} bytes: (stream, column) {_first(bad)} of {int(bad.sum())}; inside payload: {inside[bad][:5]}"
    # F4
    gm = guards.margins.cpu().numpy()
    ms = gm.shape[1]
    assert gm.shape[0] == n + 2
    assert (gm[0] == MARGIN_SENTINEL).all() and (gm[n + 1] == MARGIN_SENTINEL).all(), f"{tag} margins: guard row overwritten"
    rows = gm[1: n + 1]
    bad = (rows != MARGIN_SENTINEL) & refused[:, None]
    assert not bad.any(), f"{tag} margins: refused row written at (stream, symbol) {_first(bad)}"
    col = np.arange(ms)[None, :]
    w = min(ms, want["margins"].shape[1])
    nsym = np.minimum(want["n_symbols"], ms)
    assert int(nsym.max(initial=0)) <= w, f"{tag}: the model's margin rows are narrower than a stream's symbols"
    bad = (rows[:, :w] != want["margins"][:, :w]) & (col[:, :w] < nsym[:, None])
    assert not bad.any(), (f"{tag} margins: {int(bad.any(axis=1).sum())} streams differ, first (stream, symbol) "
                           f"{_first(bad)}; bit_frames {np.asarray(bf)[np.argwhere(bad)[:5, 0]]}, "
                           f"clock_idx {want['clock_idx'][np.argwhere(bad)[:5, 0]]}")
    if one_wave:
        K = symbols_in(lens, want["clock_idx"], bf)
        assert (want["n_symbols"] <= K).all()
        bad = (rows != MARGIN_SENTINEL) & (col >= K[:, None])
        assert not bad.any(), (f"{tag} margins: written at or beyond K, (stream, symbol) {_first(bad)}; "
                               f"K {K[np.argwhere(bad)[:5, 0]]}, bit_frames {np.asarray(bf)[np.argwhere(bad)[:5, 0]]}")
