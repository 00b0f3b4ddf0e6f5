"""The edge matrix of the live medium (tests/test_gpu_medium_ladder.py), the geometry classifier that says which piece
of kernel text decides which edge of it, and the proof that every reachable edge was placed.  Not a test module.

The medium is four kernels, each repeating the text of the one before it; ``LiveMedium.mix`` picks one per object.  A
``Case`` is a set of links over small tables, its RUNG the lowest kernel that can express it:

    0  plain     live_mix_kernel        every delay 0, no filter, no fade
    1  delayed   live_mix_delay_kernel  no filter, no fade
    2  filtered  live_mix_fir_kernel    no fade
    3  faded     live_mix_fade_kernel   always

``media`` builds one ``LiveMedium`` per rung from the case's own up to 3, a higher rung forced through the public
constructor alone (a ``filters=`` / ``fades=`` table no link names, ``max_delay=``); ``restrict`` keeps the links a
lower rung can express, so that every unfiltered path is driven by the same delays, lengths and ring residues as the
newest one.  Expected values are tests/live_fade_model.py's ``Timeline`` (one whole signal per source, no ring).

The classifier (``group_class``, ``fir_block``, ``knot_boundary``, ``history_class``) is plain integer arithmetic written
from the header comments of afsk_live_delay.hip, afsk_live_fir.hip and afsk_live_fade.hip; of the package it reads only
constants, from the kernels' source.  ``placements`` applies it to a case and ``check_ladder`` requires, from the
classifier alone, that every (consumer, class, offset) of ``required`` was placed and that nothing of ``UNREACHABLE``
was.  The consumers -- distinct pieces of kernel text that decide those classes:

    1  delay kernel, link                          5  fir kernel, first staged group
    2  fir kernel, unfiltered link                 6  fir kernel, second staged group
    3  fade kernel, unfaded unfiltered link        7  fade kernel, first staged group (unfaded and faded filtered links)
    4  fade kernel, faded unfiltered link          8  fade kernel, second staged group
    9  history kernel, behind each of the three entries ("delayed", "filtered", "faded")

Only ticks from the second on are counted: the first fills the ring with real data."""
import functools
import os
import re
from dataclasses import dataclass, field, replace

import numpy as np

from tests import live_fade_model as FD
from tests import live_mix_model as M

U = M.UNITY
Q14 = 16384
POISON = 32767
WRAP = 1 << 32


def source_constants() -> dict:
    """The constants the classifier rests on, read from the kernels' source."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "afskmodem_amd", "csrc")
    names = {"afsk_live_mix.hip": ("kMixThreads",), "afsk_live_fir.hip": ("kFirChunk", "kFirMaxTaps"),
             "afsk_live_fade.hip": ("kFadeMinShift",)}
    out = {}
    for fname, wanted in names.items():
        with open(os.path.join(csrc, fname)) as f:
            text = f.read()
        for name in wanted:
            m = re.findall(r"constexpr\s+(?:int|int32_t)\s+" + name + r"\s*=\s*(\d+)\s*[;,]", text)
            assert len(m) == 1, (name, m)
            out[name] = int(m[0])
        if fname == "afsk_live_mix.hip":
            assert len(re.findall(r"constexpr\s+int\s+kMixTile\s*=\s*kMixThreads\s*\*\s*8\s*;", text)) == 1
            out["kMixTile"] = 8 * out["kMixThreads"]
    return out


_C = source_constants()
THREADS, TILE, CHUNK, MAX_TAPS, MIN_SHIFT = (_C[k] for k in ("kMixThreads", "kMixTile", "kFirChunk", "kFirMaxTaps",
                                                             "kFadeMinShift"))


# -------------------------------------------------------------------------------------------- the geometry classifier

SILENT, SRC, RING = ("SILENT",), ("SRC",), ("RING",)


def group_class(c0: int, ln: int, pos: int, hist_len: int) -> tuple:
    """The class of the 8 timeline columns c0 ... c0 + 7 of a source with clamped length ``ln`` at medium position
    ``pos``: SILENT (c0 >= ln), SRC (wholly below the length), RING (wholly before column 0, the ring's end not inside),
    or ("EDGE", zo, lo, ro): column 0 at offset zo, the length at offset lo, the ring's end at offset ro (each 1 ... 7
    or None).  The ring's end counts among the columns that are read from the ring, those before 0."""
    if c0 >= ln:
        return SILENT
    if c0 >= 0 and c0 + 8 <= ln:
        return SRC
    h0 = (pos + c0) & (hist_len - 1)                              # the ring slot of column c0
    before = min(8, max(-c0, 0))                                  # columns of the group that lie before column 0
    to_end = hist_len - h0                                        # slots from h0 to the ring's end
    zo = -c0 if -8 < c0 < 0 else None
    lo = ln - c0 if c0 < ln < c0 + 8 else None
    ro = to_end if 0 < to_end < before else None
    if zo is None and lo is None and ro is None:
        return RING
    assert not (zo is None and lo is not None and ro is not None)
    return ("EDGE", zo, lo, ro)


def class_key(cls: tuple) -> tuple:
    """A class as ``required`` names it: single edges with their offset, the combined ones with all of theirs."""
    if cls[0] != "EDGE":
        return cls
    _, zo, lo, ro = cls
    if lo is None and ro is None:
        return ("EDGE_ZERO", zo)
    if zo is None and ro is None:
        return ("EDGE_LEN", lo)
    if zo is None and lo is None:
        return ("EDGE_RING", ro)
    if ro is None:
        return ("ZERO_LEN", zo, lo)
    if lo is None:
        return ("ZERO_RING", zo, ro)
    return ("ZERO_LEN_RING", zo, lo, ro)


def last_offset(cls: tuple) -> int:
    """The largest offset a class's edges sit at (0: none)."""
    return max([o for o in cls[1:] if o is not None], default=0) if cls[0] == "EDGE" else 0


def fir_block(tile0: int, delay: int, taps: int, ln: int, hist_len: int) -> dict:
    """The block-level facts of a filtered link in the tile that begins at column ``tile0``."""
    K = min(taps, MAX_TAPS, hist_len + 1)
    d = min(max(delay, 0), hist_len - (K - 1))
    base = tile0 - d - (K - 1)                                    # win[i] is column base + i
    Kp = -(-K // CHUNK) * CHUNK
    return dict(K=K, Kp=Kp, d=d, base=base, full=K == Kp, skip=base >= ln)


def knot_boundary(u0: int, p: int, L: int):
    """(column, kind) of the knot boundary among the 8 columns whose first has track position ``u0``: the column 0 ... 7
    whose position is a multiple of 2^p (None: none), and whether that boundary is "inner" (between two knots of the
    track), the track's "end" (back to knot 0) or the 2^32 "wrap" of the position."""
    u0 &= WRAP - 1
    j = (-u0) & ((1 << p) - 1)
    if j > 7:
        return None, None
    u = u0 + j
    if u >= WRAP:
        assert (u >> p) & (L - 1) == 0                            # (UNREACHABLE: a wrap that is not the track's end)
        return j, "wrap"
    return j, "end" if (u >> p) & (L - 1) == 0 else "inner"


def history_class(j0: int, T: int, ln: int, pos: int, hist_len: int) -> tuple:
    """The class of the 8 columns from j0 on that one thread of live_mix_history_kernel writes: ONE_SRC / ONE_ZERO (its
    one-store path, below / at or beyond the length), or ("HEDGE", to, lo, ro): T, the length, the ring's end at that
    offset of the group."""
    h0 = (pos + j0) & (hist_len - 1)
    cols = min(8, T - j0)
    to = T - j0 if j0 + 8 > T else None
    lo = ln - j0 if j0 < ln < j0 + cols else None
    ro = hist_len - h0 if 0 < hist_len - h0 < cols else None
    if to is None and lo is None and ro is None:
        return ("ONE_SRC",) if j0 + 8 <= ln else ("ONE_ZERO",)
    return ("HEDGE", to, lo, ro)


def history_key(cls: tuple) -> tuple:
    if cls[0] != "HEDGE":
        return cls
    _, to, lo, ro = cls
    single = [(n, o) for n, o in (("EDGE_T", to), ("EDGE_LEN", lo), ("EDGE_RING", ro)) if o is not None]
    return single[0] if len(single) == 1 else ("COMBINED",) + tuple(n for n, _ in single)


# ------------------------------------------------------------------------------------------------------------ a case

@dataclass(frozen=True)
class Case:
    name: str
    n_src: int
    n_out: int
    links: tuple                    # (out, src, gain, delay, filter or None, fade or None, fade offset), in row order
    filters: tuple                  # of tap tuples
    fades: tuple                    # of (knots, period)
    max_delay: int
    ticks: tuple                    # T of every mix
    lens: tuple                     # per tick: the n_src lengths as they are passed (clamped by the kernels)
    start: int                      # the position before the first mix
    noise: tuple                    # noise_scale_q24 per output row
    seed: int = 0
    meta: tuple = field(default=(), compare=False)

    @property
    def rung(self) -> int:
        return max([link_rung(x) for x in self.links], default=0)

    @property
    def hist_len(self) -> int:
        n = 8
        while n < self.max_delay:
            n *= 2
        return n

    def position(self, tick: int) -> int:
        return self.start + sum(self.ticks[:tick])

    def length(self, tick: int, s: int) -> int:
        return min(max(self.lens[tick][s], 0), self.ticks[tick])

    def tables(self) -> dict:
        """The model's keyword tables: the CSR arrays of the links as given (they are in row order)."""
        assert [x[0] for x in self.links] == sorted(x[0] for x in self.links)
        row_ptr = np.zeros(self.n_out + 1, np.int64)
        for x in self.links:
            row_ptr[x[0] + 1] += 1
        taps = [t for h in self.filters for t in h]
        return dict(row_ptr=np.cumsum(row_ptr), link_src=np.array([x[1] for x in self.links], np.int64),
                    link_gain_q15=np.array([x[2] for x in self.links], np.int64),
                    link_delay=np.array([x[3] for x in self.links], np.int64),
                    link_filter=np.array([-1 if x[4] is None else x[4] for x in self.links], np.int64),
                    filter_ptr=np.cumsum([0] + [len(h) for h in self.filters]), filter_taps=np.array(taps, np.int64),
                    link_fade=np.array([-1 if x[5] is None else x[5] for x in self.links], np.int64),
                    link_fade_offset=np.array([x[6] for x in self.links], np.int64),
                    fade_ptr=np.cumsum([0] + [len(k) for k, _ in self.fades]),
                    fade_shift=np.array([per.bit_length() - 1 for _, per in self.fades], np.int64),
                    fade_knots=np.array([v for k, _ in self.fades for v in k], np.int64))


def link_rung(x) -> int:
    return 3 if x[5] is not None else 2 if x[4] is not None else 1 if x[3] else 0


def link_kind(x) -> str:
    return {(False, False): "plain", (True, False): "filtered", (False, True): "faded",
            (True, True): "faded+filtered"}[(x[4] is not None, x[5] is not None)]


def restrict(case: Case, rung: int) -> Case:
    """``case`` with the links a medium of ``rung`` can express; a row that loses all its links goes, a row that never
    had one stays.  The sources, lengths, ticks and the start are the case's: what the history kernel sees is too."""
    had = {x[0] for x in case.links}
    keep = [x for x in case.links if link_rung(x) <= rung]
    rows = sorted({x[0] for x in keep} | (set(range(case.n_out)) - had))
    new = {r: i for i, r in enumerate(rows)}
    return replace(case, name=f"{case.name}/r{rung}", n_out=len(rows), links=tuple((new[x[0]],) + x[1:] for x in keep),
                   filters=case.filters if rung >= 2 else (), fades=case.fades if rung >= 3 else (),
                   noise=tuple(case.noise[r] for r in rows),
                   meta=tuple(m for x, m in zip(case.links, case.meta) if link_rung(x) <= rung))


def ladder(case: Case) -> list:
    """The case and its restrictions to every lower rung that still has links: what the sweep runs."""
    out = [case]
    for rung in range(case.rung - 1, -1, -1):
        sub = restrict(case, rung)
        if sub.links and sub.rung == rung:
            out.append(sub)
    return out


def subset(case: Case, rows, name: str) -> Case:
    """The rows ``rows`` of a case alone, renumbered."""
    rows = sorted(set(rows))
    new = {r: i for i, r in enumerate(rows)}
    return replace(case, name=f"{case.name}/{name}", n_out=len(rows), noise=tuple(case.noise[r] for r in rows),
                   links=tuple((new[x[0]],) + x[1:] for x in case.links if x[0] in new), meta=())


def media(case: Case, device, live=None) -> list:
    """``[(rung, LiveMedium)]`` from the case's rung up to 3, at the case's start.  Rungs 1 ... 3 get the same
    ``max_delay``; the plain medium keeps no history, and every medium a noise table (zeros where a row has none), so
    that the plain one keeps a position too."""
    if live is None:
        from afskmodem_amd import live
    out = []
    for rung in range(case.rung, 4):
        links = [x[:(3, 4, 5, 7)[rung]] for x in case.links]
        kw = dict(device=device, noise_scale_q24=np.array(case.noise, np.int32), seed=case.seed, noise_idx_base=3)
        if rung >= 1:
            kw["max_delay"] = case.max_delay
        if rung >= 2:
            kw["filters"] = [list(h) for h in case.filters] or [[Q14]]        # (a table no link names)
        if rung >= 3:
            kw["fades"] = [(list(k), per) for k, per in case.fades] or [([U], 8)]
        m = live.LiveMedium(case.n_src, case.n_out, links, **kw)
        assert (m.faded, m.filtered, m.delayed) == (rung >= 3, rung >= 2, rung >= 1), (case.name, rung)
        assert m.hist_len == (case.hist_len if rung >= 1 else 0), (case.name, rung, m.hist_len)
        t = case.tables()
        assert m.row_ptr.tolist() == t["row_ptr"].tolist() and m.link_src.tolist() == t["link_src"].tolist()
        assert m.link_gain_q15.tolist() == t["link_gain_q15"].tolist()
        assert m.link_delay.tolist() == t["link_delay"].tolist() and m.link_filter.tolist() == t["link_filter"].tolist()
        assert m.link_fade.tolist() == t["link_fade"].tolist()
        assert m.link_fade_offset.tolist() == t["link_fade_offset"].tolist()
        if case.filters and rung >= 2:
            assert m.filter_ptr.tolist() == t["filter_ptr"].tolist() and m.filter_taps.tolist() == t["filter_taps"].tolist()
        if case.fades and rung >= 3:
            assert m.fade_ptr.tolist() == t["fade_ptr"].tolist() and m.fade_knots.tolist() == t["fade_knots"].tolist()
            assert m.fade_shift.tolist() == t["fade_shift"].tolist()
        m.reset(case.start)
        out.append((rung, m))
    return out


def sources(case: Case, tick: int) -> np.ndarray:
    """int16 [n_src, T + 3]: different random data in every row, POISON from the source's clamped length on -- the
    columns up to T the kernels must not hear and the ones past T they must not read."""
    T = case.ticks[tick]
    root = case.name.split("/")[0]                               # a restriction hears what its case hears
    rng = np.random.default_rng([sum(root.encode()), len(root), case.start & 0xFFFF, tick])
    host = rng.integers(-32768, 32768, (case.n_src, T + 3), dtype=np.int16)
    host[host == 0] = 1
    for s in range(case.n_src):
        host[s, case.length(tick, s):] = POISON
    return host


def run_model(case: Case, tables=None, src_lens="case", before_tick=None, timeline=FD.Timeline):
    """``(rows per tick, the ring after every tick, the position after every tick)`` of the model over the case's own
    tables, or over ``tables``.  ``src_lens`` None: the lengths are not passed (every source counts for T columns).
    ``before_tick(tl, tick)`` may touch the timeline before a mix.  The ring is the model's timeline laid out as the
    header defines the history -- time t at slot t & (hist_len - 1), zeros before the start: nothing of it is computed
    through a ring."""
    t = case.tables() if tables is None else tables
    if timeline is not FD.Timeline:                               # the delayed or the filtered model: fewer tables
        t = {k: v for k, v in t.items() if k in timeline.mix.__code__.co_varnames}
    tl = timeline(case.n_src, case.hist_len, case.start)
    rows, rings, poss = [], [], []
    H = case.hist_len
    for tick, T in enumerate(case.ticks):
        if before_tick is not None:
            before_tick(tl, tick)
        lens = None if src_lens is None else list(case.lens[tick])
        rows.append(tl.mix(sources(case, tick), n_out=case.n_out, T=T, src_lens=lens,
                           noise_scale_q24=np.array(case.noise, np.int64), seed=case.seed, noise_idx_base=3, **t))
        ring = np.zeros((case.n_src, H), np.int16)
        held = tl.X[:, -H:]
        times = tl.pos - held.shape[1] + np.arange(held.shape[1])
        ring[:, times & (H - 1)] = held
        rings.append(ring)
        poss.append(tl.pos)
    return rows, rings, poss


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """``run_model`` of the registered case ``name``, computed once per process."""
    return run_model(CASES[name])


# -------------------------------------------------------------------------------------------------------- placements

def link_taps(case: Case, x) -> int:
    return len(case.filters[x[4]])


def placements(case: Case) -> dict:
    """{(part, fact): [(tick, row), ...]} of the ticks from the second on.  Parts: "U" an unfaded unfiltered link's
    groups, "UF" a faded unfiltered link's, "S1" / "S2" a filtered link's first / second staged groups ("S1f" / "S2f":
    the link is faded too), "H" the history kernel's groups (row: the source).  Facts: ("class", key) with
    ``class_key`` / ``history_key``; for S parts ("tile 1", key) -- the first group of tile 1 --, ("full", bool) --
    K == Kp --, ("skip", bool), ("restage",) and for S2 ("tile", its tile); for faded links ("knot", column), ("kind",
    boundary kind), and for UF ("knot+edge", column): a boundary in a group whose class is an edge.  A group counts where what it decides reaches an output column: an unfiltered group's edges below T, a
    staged group wholly inside the columns some output column's taps read."""
    H = case.hist_len
    out = {}

    def put(part, fact, tick, row):
        out.setdefault((part, fact), []).append((tick, row))

    rows = {}
    for x in case.links:
        rows.setdefault(x[0], []).append(x)
    for tick in range(1, len(case.ticks)):
        T, pos = case.ticks[tick], case.position(tick)
        tiles = -(-T // TILE)
        for row, links in rows.items():
            for tile in range(tiles):
                tile0 = tile * TILE
                Tt = min(T - tile0, TILE)
                staged = False
                for x in links:
                    _, s, _, delay, filt, fade, off = x
                    ln = case.length(tick, s)
                    track = None
                    if fade is not None:
                        knots, per = case.fades[fade]
                        track = (max(per.bit_length() - 1, MIN_SHIFT), len(knots))
                    if filt is None:
                        d = min(max(delay, 0), H)
                        part = "U" if fade is None else "UF"
                        for j0 in range(tile0, tile0 + Tt, 8):
                            cls = group_class(j0 - d, ln, pos, H)
                            seen = min(8, T - j0)                 # the group's columns that are output
                            if last_offset(cls) < seen and (cls[0] == "EDGE" or seen == 8):
                                put(part, ("class", class_key(cls)), tick, row)
                            if track:
                                col, kind = knot_boundary(pos + j0 + off, *track)
                                if col is not None and col < seen:
                                    put(part, ("knot", col), tick, row)
                                    put(part, ("kind", kind), tick, row)
                                    if cls[0] == "EDGE" and last_offset(cls) < seen:
                                        put(part, ("knot+edge", col), tick, row)
                        continue
                    b = fir_block(tile0, delay, link_taps(case, x), ln, H)
                    f = "" if fade is None else "f"
                    put("S1" + f, ("skip", b["skip"]), tick, row)
                    if b["skip"]:
                        continue
                    put("S1" + f, ("full", b["full"]), tick, row)
                    if staged:
                        put("S1" + f, ("restage",), tick, row)
                    used = Tt + b["K"] - 1                        # win[0 ... used) reach an output column
                    second = False
                    for i0 in range(0, min(TILE + b["Kp"], used - 7), 8):
                        part = ("S1" if i0 < TILE else "S2") + f
                        key = class_key(group_class(b["base"] + i0, ln, pos, H))
                        put(part, ("class", key), tick, row)
                        if tile > 0 and i0 == 0:
                            put(part, ("tile 1", key), tick, row)     # the first group of a tile behind the first
                        second |= i0 >= TILE
                    if second:
                        put("S2" + f, ("tile", tile), tick, row)
                        put("S2" + f, ("full", b["full"]), tick, row)
                        put("S2" + f, ("skip", False), tick, row)
                        if staged:
                            put("S2" + f, ("restage",), tick, row)
                    staged = True
                    if track:
                        for j0 in range(tile0, tile0 + Tt, 8):
                            col, kind = knot_boundary(pos + j0 + off, *track)
                            if col is not None and col < min(8, T - j0):
                                put("S1f", ("knot", col), tick, row)
                                put("S1f", ("kind", kind), tick, row)
        first = max(T - H, 0)
        put("H", ("first", "0" if first == 0 else "T-hist_len"), tick, -1)
        for s in range(case.n_src):
            for j0 in range(first, T, 8):
                put("H", ("class", history_key(history_class(j0, T, case.length(tick, s), pos, H))), tick, s)
    return out


def consumers_of(part: str, rung: int) -> list:
    """The consumers a part of a case of ``rung`` reaches: the case runs on every medium from its rung up."""
    reach = range(rung, 4)
    if part == "U":
        return [c for c, r in ((1, 1), (2, 2), (3, 3)) if r in reach]
    if part == "UF":
        return [4]
    if part in ("S1", "S2"):
        first = part == "S1"
        return [c for c, r in ((5 if first else 6, 2), (7 if first else 8, 3)) if r in reach]
    if part in ("S1f", "S2f"):
        return [(7 if part == "S1f" else 8, "faded")]
    assert part == "H"
    return [(9, e) for e, r in (("delayed", 1), ("filtered", 2), ("faded", 3)) if r in reach]


def placed(cases) -> dict:
    """{(consumer, fact): [case names]} over ``cases``.  A faded filtered link's classes count for consumers 7 and 8
    like an unfaded one's; its own facts are kept under (7, "faded") / (8, "faded")."""
    out = {}
    for case in cases:
        for (part, fact), where in placements(case).items():
            for c in consumers_of(part, case.rung):
                out.setdefault((c, fact), []).append(case.name)
                if isinstance(c, tuple) and c[0] in (7, 8) and fact[0] not in ("knot", "kind"):
                    out.setdefault((c[0], fact), []).append(case.name)
    return out


OFFSETS = range(1, 8)
MIX_CLASSES = [SILENT, SRC, RING] + [(n, o) for n in ("EDGE_ZERO", "EDGE_LEN", "EDGE_RING") for o in OFFSETS]
HISTORY_CLASSES = [("ONE_SRC",), ("ONE_ZERO",)] + [(n, o) for n in ("EDGE_T", "EDGE_LEN", "EDGE_RING") for o in OFFSETS]

# What cannot be placed, with its arithmetic; ``check_ladder`` fails if one of these was placed after all.
UNREACHABLE = {
    "LEN_RING": "the length and the ring's end in one group without column 0: the ring is read for columns below 0 and "
                "the length is at least 0, so column 0 lies between the two",
    (6, ("skip", True)): "a skipped block (base >= len) stages no group at all, so no second one",
    (8, ("skip", True)): "as consumer 6: live_mix_fade_kernel skips the block before it stages",
    "S2 beyond tile 0": "a second staged group is read by an output column only where the tile's columns plus K - 1 "
                        "exceed 2048 + 8; with T <= 2072 tile 1 has at most 24 columns and 24 + 255 < 2056",
    "wrap not end": "the 2^32 wrap of the track position that is not also the track's end: a track's period L * 2^p is "
                    "a power of two of at most 2^31 and divides 2^32, so knot 0 begins where the position wraps",
    "offset mod 2^31": "an envelope offset taken modulo 2^31 changes no sample: the period divides 2^31 as well",
}


def required() -> list:
    req = []
    for c in range(1, 9):
        req += [(c, ("class", k)) for k in MIX_CLASSES]
        req += [(c, ("combined", n)) for n in ("ZERO_LEN", "ZERO_RING")]
    for c in (5, 6, 7, 8):
        req += [(c, ("full", True)), (c, ("full", False)), (c, ("skip", False)), (c, ("restage",))]
    req += [(c, ("skip", True)) for c in (5, 7)]
    req += [(c, ("tile 1", k)) for c in (5, 7) for k in MIX_CLASSES[3:]]
    req += [(4, ("knot+edge", col)) for col in range(8)] + [(4, ("kind", k)) for k in ("inner", "end", "wrap")]
    req += [((7, "faded"), ("knot", col)) for col in range(8)]
    req += [((7, "faded"), ("kind", k)) for k in ("inner", "end", "wrap")]
    req += [((7, "faded"), ("full", v)) for v in (True, False)] + [((8, "faded"), ("class", ("EDGE_ZERO", 1)))]
    for e in ("delayed", "filtered", "faded"):
        req += [((9, e), ("class", k)) for k in HISTORY_CLASSES]
        req += [((9, e), ("first", v)) for v in ("0", "T-hist_len")]
    return req


def check_ladder(cases) -> dict:
    """Every requirement placed, nothing unreachable placed; returns ``placed(cases)``."""
    got = placed(cases)
    for key in list(got):                                         # the combined classes, whatever their offsets
        c, fact = key
        if fact[0] == "class" and fact[1][0] in ("ZERO_LEN", "ZERO_RING", "ZERO_LEN_RING"):
            for n in ("ZERO_LEN", "ZERO_RING"):
                if all(w in fact[1][0] for w in n.split("_")):
                    got.setdefault((c, ("combined", n)), []).extend(got[key])
    missing = [r for r in required() if r not in got]
    assert not missing, (len(missing), missing[:12])
    for key in UNREACHABLE:
        if isinstance(key, tuple):
            assert key not in got, (key, got[key][:3])
        else:                                                     # (the others are asserted where they would show:
            assert key in ("LEN_RING", "S2 beyond tile 0", "wrap not end", "offset mod 2^31")   # group_class,
    assert not [k for k in got if k[1][0] == "tile" and k[1][1] > 0]                    # knot_boundary, the host test)
    return got


# ------------------------------------------------------------------------------------------------------- the cases

SMALL_HIST = (8, 16)
SMALL_TICKS = (24, 24, 7, 1, 24)
SMALL_KS = (1, 2, 3, 8, 9, 15, 16, 17)
WRAP_STARTS = (WRAP - 5, WRAP - 29)    # the position wraps 5 columns into tick 0, and 5 columns into tick 1
GAINS = (U, -U, 65535, U // 2, -65535)
FADE_OFFSETS = (0, 1, 2, 3, 4, 5, 6, 7, (1 << 31) + 3, WRAP - 2, (1 << 31) + 17)
SMALL_FADES = (((40000,), 8), ((65535, 3000, 20000, 32768), 8))     # p = 3; L = 1 and 4


def lengths_of(T: int) -> tuple:
    """Below 0, 0, 1, 7, 8, 9, T - 1, T, above T."""
    return (-3, 0, 1, 7, 8, 9, T - 1, T, T + 5)


def taps_of(K: int) -> tuple:
    """K taps whose magnitudes sum to at most 65535, the first and the last not 0."""
    top = min(32767, 65535 // K)
    h = np.random.default_rng(K).integers(-top, top + 1, K)
    h[0], h[-1] = top, -top
    return tuple(int(t) for t in h)


def small_starts(hist_len: int) -> tuple:
    return tuple(range(hist_len)) + WRAP_STARTS


def small_case(hist_len: int, start: int) -> Case:
    """One row per link: every source (one per length), every delay 0 ... hist_len, the four kinds, every K that fits.
    Tick 0 fills the ring at full lengths, tick 1 has the lengths, ticks 2 and 3 are the short ones, tick 4 reads what
    they left with the lengths moved on by four sources."""
    links, meta = [], []
    ks = [K for K in SMALL_KS if K - 1 <= hist_len]
    for s in range(9):
        for d in range(hist_len + 1):
            for K in [None] + [K for K in ks if d + K - 1 <= hist_len]:
                for faded in (False, True):
                    k = len(links)
                    links.append((k, s, GAINS[k % len(GAINS)], d, None if K is None else ks.index(K),
                                  k // 2 % 2 if faded else None, FADE_OFFSETS[k % len(FADE_OFFSETS)] if faded else 0))
                    meta.append(dict(s=s, d=d, K=K, faded=faded))
    T = SMALL_TICKS
    turned = lengths_of(T[4])
    lens = ((T[0],) * 9, lengths_of(T[1]), lengths_of(T[2]), lengths_of(T[3]), turned[4:] + turned[:4])
    return Case(f"small-h{hist_len}-p{start}", 9, len(links), tuple(links), tuple(taps_of(K) for K in ks), SMALL_FADES,
                hist_len, T, lens, start, (0,) * len(links), meta=tuple(meta))


ROWS_TICKS = (24, 9, 10, 11, 12, 13, 14, 15, 24)      # below hist_len 16: the history kernel's last group straddles T


def rows_case() -> Case:
    """Rows of degree 0, 2 and 5 that mix the kinds, gains +-UNITY, 65535 and 0, noise on two rows; ticks that end at
    every offset of the history kernel's last group, and lengths at every offset of its first."""
    links = [(1, 0, U, 0, None, None, 0), (1, 1, -U, 0, None, None, 0),
             (2, 2, 65535, 5, None, None, 0), (2, 0, U, 2, 0, None, 0),
             (3, 0, U, 0, None, None, 0), (3, 1, -U, 16, None, None, 0), (3, 2, 65535, 3, 1, None, 0),
             (3, 3, 0, 1, None, 0, 5), (3, 3, U // 2, 2, 0, 1, WRAP - 9),
             (4, 0, U, 0, None, None, 0), (4, 1, -U, 0, None, None, 0), (4, 2, 65535, 0, None, None, 0),
             (4, 3, 0, 0, None, None, 0), (4, 0, U // 3, 0, None, None, 0),
             (5, 1, U, 9, None, 1, 3), (5, 2, -U, 4, 1, 0, 2)]
    lens = tuple((tick % 8, 8 + (tick + 3) % 8, T - 1, T) for tick, T in enumerate(ROWS_TICKS))
    return Case("rows", 4, 6, tuple(links), (taps_of(3), taps_of(9)), SMALL_FADES, 16, ROWS_TICKS, lens, 13,
                (0, 1 << 20, 0, 5 << 20, 0, 0), seed=11)


TILE_HIST = 4096
TILE_T = TILE + 24
TILE_START = 4051                       # position 2027 mod 4096 at tick 1, 3 at tick 2
TILE_KS = (16, 17, 255, 256)
TILE_ENDS = tuple(TILE + 8 + o for o in OFFSETS)
TILE_LENS = ((TILE_T,) * 11, (TILE_T, 100, 0, TILE_T) + TILE_ENDS, (TILE_T, 100, 5, 0) + TILE_ENDS)


def tile_case() -> Case:
    """hist_len 4096, T = 2048 + 24.  The column 2048 - reach (reach = d + K - 1) is both the first column of tile 0's
    second staged group and of tile 1's first one; the reaches put column 0, the ring's end (tick 1: position 2027 mod
    4096) and the length of source 1 (100) at every offset of it, both sides of tile 1's skip (base 99, 100, 101
    against the length 100), column 0 and the ring's end in one group (tick 2: position 3 mod 4096), column 0 and the
    length in one group (source 2 at tick 1 and source 3 at tick 2 have length 0 behind a full tick, so the ring they
    are heard from holds data; source 2 at tick 2 has length 5).  Sources 4 ... 10 end 1 ... 7 columns into the group at
    2056."""
    specs = [(3 + o, TILE + o) for o in OFFSETS]                                   # EDGE_ZERO(o); tick 2: with the ring's end
    specs += [(0, 2 * TILE - 21 + o) for o in OFFSETS]                             # EDGE_RING(o) at tick 1
    specs += [(0, 3000), (0, None)]                                                # RING; SRC (delay 0)
    specs += [(1, TILE - 100 + o) for o in (-1, 0) + tuple(OFFSETS)]               # the skip's boundary; EDGE_LEN(o)
    specs += [(s, TILE + o) for s in (2, 3) for o in OFFSETS]                      # column 0 and the length
    links, noise = [], []
    for K in TILE_KS:
        for s, reach in specs:
            for faded in (False, True):
                k = len(links)
                d = 0 if reach is None else reach - (K - 1)
                links.append((k, s, GAINS[k % len(GAINS)], d, TILE_KS.index(K), k // 2 % 2 if faded else None,
                              FADE_OFFSETS[k % len(FADE_OFFSETS)] if faded else 0))
                noise.append((1 << 20) if k % 37 == 5 else 0)
    for s in range(4, 11):                                         # unfiltered links that read the ends sources 4 ... 10 left
        for faded in (False, True):
            k = len(links)
            links.append((k, s, GAINS[k % len(GAINS)], 24, None, 1 if faded else None, k if faded else 0))
            noise.append(0)
    r = len(links)
    links += [(r, 0, U // 2, TILE + 2 - 254, 2, None, 0), (r, 4, U // 2, TILE + 3 - 15, 0, 1, 6),      # back to back
              (r + 1, 3, U, 0, 1, None, 0), (r + 1, 0, -U, TILE + 5 - 16, 1, None, 0),                # behind a skipped one
              (r + 2, 5, U // 2, 24, None, None, 0), (r + 2, 0, U // 4, TILE + 4 - 255, 3, None, 0),  # behind an unfiltered
              (r + 2, 0, U // 4, 2100, None, 0, 4), (r + 2, 6, -U // 4, TILE + 1 - 15, 0, 0, 1)]
    noise += [3 << 20, 0, 1 << 20]
    return Case("tile", 11, r + 3, tuple(links), tuple(taps_of(K) for K in TILE_KS), SMALL_FADES, TILE_HIST,
                (TILE_T,) * 3, TILE_LENS, TILE_START, tuple(noise), seed=4)


def base_names() -> list:
    return [f"small-h{h}-p{p}" for h in SMALL_HIST for p in small_starts(h)] + ["rows", "tile"]


class _Cases(dict):
    """name -> Case, built when first asked for; ``name/rK`` is the restriction to rung K."""

    def __missing__(self, name):
        root, _, sub = name.partition("/")
        if sub:
            case = restrict(self[root], int(sub[1:]))
        elif root == "rows":
            case = rows_case()
        elif root == "tile":
            case = tile_case()
        else:
            h, p = re.fullmatch(r"small-h(\d+)-p(\d+)", root).groups()
            case = small_case(int(h), int(p))
        assert case.name == name
        self[name] = case
        return case


CASES = _Cases()


def ladder_names(base: str) -> list:
    return [c.name for c in ladder(CASES[base])]


def all_cases() -> list:
    return [CASES[n] for b in base_names() for n in ladder_names(b)]


def locate(case: Case, tick: int, row: int) -> list:
    """What the classifier says about output row ``row`` at ``tick``: the (part, fact) pairs it was placed for."""
    return sorted({(part, fact) for (part, fact), where in placements(case).items() if (tick, row) in where}, key=str)
