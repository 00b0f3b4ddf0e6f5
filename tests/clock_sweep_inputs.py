"""Input sets of the clock-recovery sweeps (tests/test_gpu_clock_sweeps.py) and the placement conditions each set
was built for.  Not a test module.

Clock recovery (ref:322-339) returns the first offset i in [0, 4096 - 2 bf) whose truncated mean total(i) // (2 bf)
is minimal.  The device computes it in five forms (lanes, lane steps, run-time, the total(0) < N shortcut, the rate
detector's prefix sums); clean transmissions only ever tie at exact zeros and noise never ties at all, so these sets
put the decision where the forms differ: totals exactly on and one below a bin edge, equal means at different totals,
winners on both sides of every lane and step seam, at the first and the last searched offset and just outside, and
means at the top of the 16-bit quotient range.  Write N = 2 bf and NOFF = 4096 - N.

  (A) a bump on silence: every offset has total 65535 bf (mean 32767); ONE sample, at the last high position of the
      template laid at p, is v.  v = bf puts total(p) exactly on 32767 N -- the same bin, the earlier tie wins --,
      v = bf + 1 one below it -- the next bin, p wins.  Offset 0 must not see the bump for that, p >= bf / 2 + 1, which
      no offset of bit_frames 1920 and above can meet; the mirrored bump, -v at the template's very last position,
      is seen by no offset before p and separates at every rate.
  (B) pockets on silence: one exact training cycle at p with its first sample lowered by d, total(p) = d.  Singly at
      every seam of the form that owns the rate, at the first and last two offsets and at NOFF, NOFF + 1 (outside the
      search); in pairs with equal and with neighbouring means.
  (C) transmissions at level 20000 that decode: every aligned cycle has total = bf (mod N) at mean 12767; the first
      sample of one cycle raised or lowered by bf - 1, bf, bf + 1 moves the winner from cycle to cycle.
  (D) the inverted cycle tiled at full scale: aligned offsets reach 65535 N, the largest quotient there is.

Every set is a ``split_sweep_inputs.Sweep``; the expected outputs are the oracle's.  The ``check_*`` functions assert,
from the oracle's outputs and the numpy model of the totals (tests/detect_model.py), that every placement happened
and that each of six wrong rules (``WRONG_RULES``) would have answered differently on at least one stream of every
rate.  tests/test_clock_sweep_inputs_host.py runs them on the CPU; the GPU sweeps run them again on the very data
they compare."""
import functools
import os
import re

import numpy as np

from tests import detect_model as DM
from tests import split_sweep_inputs as I
from tests import symbol_streams as G

WINDOW = G.SYNC_WINDOW
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "afskmodem_amd", "csrc")

# run-time geometries: 28 the smallest (q = 7, odd), 1028 with q odd, 2044 with NOFF = 8
RT_RATES = (28, 36, 44, 124, 132, 516, 964, 1028, 2040, 2044)
# compile-time rates that ALSO run the run-time form: the split path (8, 100, 2000) and the streaming live receiver
ALSO_RT = (8, 100, 2000)
LEVEL = 20000                       # family C: above both gates' thresholds, far below full scale
C_MAX_BF = 680                      # two aligned cycles in the window: 2 N + 8 <= NOFF
PAIR_DS = ("same_bin_later_smaller", "next_bin_later", "same_bin_far")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def source_constants():
    """What the placements depend on, read from the kernel sources: the two lists of compile-time geometries, the
    offsets a lane owns in each form, the step, and the largest bit_frames of the lanes form."""
    impl, sync, rt, fast = (_read(n) for n in ("afsk_demod_impl.h", "afsk_demod_sync.h", "afsk_demod_rt.h",
                                               "afsk_demod_fast.h"))
    lists = {}
    for name in ("AFSK_FAST_BF_LIST", "AFSK_GP_BF_LIST"):
        m = re.findall(r"#define\s+" + name + r"\(X\)((?:\s*X\(\d+\))+)\s*$", impl, re.M)
        assert len(m) == 1, name
        lists[name] = tuple(int(v) for v in re.findall(r"X\((\d+)\)", m[0]))
    lanes_gc = re.findall(r"static constexpr int GC = (\d+);", sync)
    steps = re.findall(r"constexpr int GC = (\d+), STEP = (\d+) \* GC, T =", sync)
    rt_gc = re.findall(r"constexpr int GC = (\d+), STEP = (\d+) \* GC;", rt)
    lanes_max = re.findall(r"constexpr bool LANES_FORM = BF <= (\d+);", fast)
    assert len(lanes_gc) == 1 and len(steps) == 1 and len(rt_gc) == 1 and len(lanes_max) == 1
    return dict(fast=lists["AFSK_FAST_BF_LIST"], gp=lists["AFSK_GP_BF_LIST"], lanes_gc=int(lanes_gc[0]),
                steps_gc=int(steps[0][0]), step=int(steps[0][0]) * int(steps[0][1]), rt_gc=int(rt_gc[0][0]),
                rt_step=int(rt_gc[0][0]) * int(rt_gc[0][1]), lanes_max=int(lanes_max[0]))


def compiled_rates():
    c = source_constants()
    return tuple(sorted(c["fast"] + c["gp"]))


def rates():
    """All 46: the 36 compile-time geometries and the ten run-time values."""
    return tuple(sorted(compiled_rates() + RT_RATES))


def form(bf):
    """The form a batch kernel recovers this rate's clock with."""
    if bf not in compiled_rates():
        return "rt"
    return "lanes" if bf <= source_constants()["lanes_max"] else "steps"


def forms(bf):
    return (form(bf),) + (("rt",) if bf in ALSO_RT else ())


def gc_of(f):
    c = source_constants()
    return {"lanes": c["lanes_gc"], "steps": c["steps_gc"], "rt": c["rt_gc"]}[f]


def seams(bf):
    """The first offset of every lane run and step the rate's forms hand from one owner to the next: 72 l for l = 1
    and l = LANES - 1; 24 l for l = 1 and l = 63, and every 1536 t.  Not restricted to [0, NOFF)."""
    c = source_constants()
    NOFF = WINDOW - 2 * bf
    out = set()
    for f in forms(bf):
        if f == "lanes":
            lanes = -(-NOFF // c["lanes_gc"])
            out |= {c["lanes_gc"], c["lanes_gc"] * (lanes - 1)}
        else:
            out |= {gc_of(f), gc_of(f) * 63} | {c["step"] * t for t in range(1, -(-NOFF // c["step"]))}
    return sorted(out)


def placements(bf):
    """Family B's single-pocket offsets inside the search."""
    NOFF = WINDOW - 2 * bf
    ps = {0, 1, NOFF - 2, NOFF - 1} | {s + e for s in seams(bf) for e in (-1, 0, 1)}
    return sorted(p for p in ps if 0 <= p < NOFF)


def pair_placements(bf):
    """{class: (p1, p2)} of family B's two pockets, for the classes the geometry allows."""
    N, NOFF = 2 * bf, WINDOW - 2 * bf
    c = source_constants()
    out = {}
    if 2 * N + 8 > NOFF:
        return out
    for f in forms(bf):
        gc = gc_of(f)
        if N <= gc - 1:                                     # both inside the run of lane 2
            out["B2_lane_" + f] = (2 * gc, 2 * gc + N)
    gc = gc_of(form(bf))
    out["B2_near"] = (3 * gc - 1, 3 * gc - 1 + N)           # the last offset of lane 2, and the nearest disjoint cycle
    if N <= c["step"] and c["step"] + 29 < NOFF:
        out["B2_step"] = (29, 29 + c["step"])               # the same lane (1 of the 24-offset forms), the next step
    return out


def expected_missing():
    """{class: rates} that geometry rules out, from the inequalities alone (the CPU suite holds MISSING and the
    generator's output against this)."""
    c = source_constants()
    out = {"B2_lane": [], "B2_near": [], "B2_step": [], "C": []}
    for bf in rates():
        N, NOFF = 2 * bf, WINDOW - 2 * bf
        two = 2 * N + 8 <= NOFF
        if not (two and any(N <= gc_of(f) - 1 for f in forms(bf))):
            out["B2_lane"].append(bf)
        if not two:
            out["B2_near"].append(bf)
        if not (two and N <= c["step"] and c["step"] + 29 < NOFF):
            out["B2_step"].append(bf)
        if not two:
            out["C"].append(bf)
    return {k: tuple(v) for k, v in out.items()}


_ABOVE_680 = (800, 960, 964, 1000, 1028, 1200, 1500, 1600, 1920, 2000, 2040, 2044)
# (class, rate) pairs that geometry rules out.  Two pockets in ONE lane's run need N below the run (72 offsets in the
# lanes form, 24 in the others): bit_frames 4 ... 32 of the lanes form.  Two disjoint cycles, and two aligned cycles
# of a transmission, need 2 N + 8 <= NOFF: bit_frames <= 680.  Families A, D and the single pockets exist everywhere.
MISSING = {
    "B2_lane": (28, 36, 40, 44, 48, 60, 64, 80, 96, 100, 120, 124, 128, 132, 160, 192, 200, 240, 300, 320, 384, 400,
                480, 500, 516, 600, 640) + _ABOVE_680,
    "B2_near": _ABOVE_680,
    "B2_step": _ABOVE_680,
    "C": _ABOVE_680,
}


def classes_of(bf):
    """The classes a rate's sweep must hold."""
    return sorted({"A", "B1", "B_outside", "D"} | {k for k, v in MISSING.items() if bf not in v})


# ------------------------------------------------------------------------------------------------ the generator

def stream_len(bf):
    """4096 + 2 N: samples past the sync window exist, so a window one too long sees them."""
    return WINDOW + 4 * bf


def a_offsets(bf, sign):
    """Family A's offsets p: first, middle and last for the positive bump, the same with 1 for 0 for the negative
    one (at p = 0 nothing lies before p to tie with)."""
    NOFF = WINDOW - 2 * bf
    return (0, NOFF // 2, NOFF - 1) if sign > 0 else (1, NOFF // 2, NOFF - 1)


def cycle(bf):
    return DM.training_cycle(bf).astype(np.int16)


def pocket(x, bf, p, d):
    """One exact training cycle at offset p, its first sample lowered by d: total(p) = d."""
    x[p: p + 2 * bf] = cycle(bf)
    x[p] = DM.HI - d
    return x


def tones(bf):
    """int32 [2, bf] (space, mark): the oracle's for a rate a Receiver can have, the halves of the training cycle
    (which are those, tests/test_clock_sweep_inputs_host.py) for the others."""
    if 48000 % bf == 0:
        return G.tones(bf)
    tc = DM.training_cycle(bf)
    return np.stack([tc[bf:], tc[:bf]]).astype(np.int32)


def render(bits, bf, level, lead):
    """``symbol_streams.render``, also for a bit_frames that does not divide 48000."""
    if 48000 % bf == 0:
        return G.render(bits, bf, level, lead)
    b = np.asarray(bits, np.int64)
    sym = tones(bf)[b]
    for k, (a, d) in level.items():
        s = np.sign(sym[k]) * int(a)
        s[0] = int(a) + int(d)
        sym[k] = s
    return np.concatenate([np.zeros(int(lead), np.int32), sym.reshape(-1)]).astype(np.int16)


def c_cycles(bf, lead):
    """Aligned cycles of a family-C stream whose offsets lie inside the search."""
    return (WINDOW - 2 * bf - 1 - lead) // (2 * bf) + 1


C_LEADS = (2, 73)                   # both parities, one behind the first lane of the lanes form
# (cycle, change of its first sample in units (bf, +-1)) ...: and the aligned cycle that then wins
C_VARIANTS = (
    ("raise_on_edge", lambda bf, c: {c: bf}, lambda c: 0),
    ("raise_past_edge", lambda bf, c: {c: bf + 1}, lambda c: c),
    ("lower_inside", lambda bf, c: {0: -(bf - 1)}, lambda c: 0),
    ("lower_on_edge", lambda bf, c: {0: -bf}, lambda c: 1),
    ("lower_two", lambda bf, c: {0: -bf, 1: -bf}, lambda c: 2),
)


def family_c(bf, rng, payload=2):
    out = []
    for i, (name, change, winner) in enumerate(C_VARIANTS):
        lead = C_LEADS[i % 2]
        n = c_cycles(bf, lead)
        assert n >= 3, (bf, lead)
        train = G.training(min(n, 8))
        bits = train + G.coded(bytes(rng.integers(0, 256, payload, dtype=np.uint8)))
        c = 1 + i % 2
        level = {k: (LEVEL, 0) for k in range(len(bits))}
        for cyc, d in change(bf, c).items():
            level[2 * cyc] = (LEVEL, d)
        x = render(bits, bf, level, lead)
        x = np.concatenate([x, np.zeros(max(12 * bf, stream_len(bf) - len(x)), np.int16)])
        out.append((x, dict(fam="C", cls="C", variant=name, lead=lead, win=lead + winner(c) * 2 * bf)))
    return out


@functools.lru_cache(maxsize=None)
def sweep(bf):
    """Every stream of one rate."""
    N, NOFF, L = 2 * bf, WINDOW - 2 * bf, stream_len(bf)
    rng = np.random.default_rng(7000 + bf)
    rows = []
    silence = lambda: np.zeros(L, np.int16)  # noqa: E731
    # (A) a positive bump under the template's last high position, a negative one under its last position
    for p in a_offsets(bf, 1):
        for v in (bf, bf + 1):
            x = silence()
            x[p + bf + bf // 2 - 1] = v
            rows.append((x, dict(fam="A", cls="A", sign=1, p=p, v=v)))
    for p in a_offsets(bf, -1):
        for v in (bf, bf + 1):
            x = silence()
            x[p + N - 1] = -v
            rows.append((x, dict(fam="A", cls="A", sign=-1, p=p, v=v)))
    # (B) single pockets, inside the search and just outside
    for p in placements(bf) + [NOFF, NOFF + 1]:
        for d in (0, 5):
            rows.append((pocket(silence(), bf, p, d), dict(fam="B1", cls="B1" if p < NOFF else "B_outside", p=p, d=d)))
    # (B) two pockets
    ds = dict(zip(PAIR_DS, ((N + 3, N, 0), (N, N - 1, 1), (2 * N - 1, N, 0))))
    for cls, (p1, p2) in pair_placements(bf).items():
        assert p2 - p1 >= N and p2 < NOFF
        for name, (d1, d2, win) in ds.items():
            x = pocket(pocket(silence(), bf, p1, d1), bf, p2, d2)
            rows.append((x, dict(fam="B2", cls=cls, pair=name, p1=p1, p2=p2, win=(p1, p2)[win])))
    # (C)
    if bf <= C_MAX_BF:
        rows += family_c(bf, rng)
    # (D) the inverted cycle tiled from sample `phase` on (and before it): with a pocket, and without one at phase 0
    # (offset 0 is aligned: the total the step forms start from) and at phase 24 (lane 1's first offset)
    inv = ~cycle(bf)
    pd = min((NOFF // 2) | 1, NOFF - 1)
    for phase, p in ((0, pd), (0, None), (24, None)):
        x = inv[(np.arange(L) - phase) % N]
        if p is not None:
            x = pocket(x, bf, p, 5)
        rows.append((x, dict(fam="D", cls="D", phase=phase, p=-1 if p is None else p)))
    for x, _ in rows:
        assert x.dtype == np.int16 and len(x) >= L
    return I.assemble([(x, bf, m) for x, m in rows])


def sweep_of(bfs):
    """The sweeps of several rates as one batch."""
    out = None
    for bf in bfs:
        out = sweep(bf) if out is None else I.concat(out, sweep(bf))
    return out


@functools.lru_cache(maxsize=None)
def sweep_all():
    return sweep_of(rates())


def oracle(sw):
    return I.oracle(sw)


@functools.lru_cache(maxsize=None)
def load_all():
    """(the whole sweep, the oracle's outputs): computed once per process and left unchanged."""
    sw = sweep_all()
    want = oracle(sw)
    for a in want.values():
        a.setflags(write=False)
    return sw, want


def window_of(sw, s):
    o = int(sw.off[s])
    return sw.flat[o: o + int(sw.ln[s])]


# ------------------------------------------------------------------------------------------------ the wrong rules

def total_at(x, bf, i):
    return int(np.abs(DM.training_cycle(bf) - np.asarray(x[i: i + 2 * bf], np.int64)).sum())


def first_minimum(x, bf):
    """The definition, on the numpy model's totals."""
    return int(np.argmin(DM.totals(x, bf) // (2 * bf)))


def wrong_rules(x, bf):
    """What six defective searches would answer for the stream x."""
    N = 2 * bf
    t = DM.totals(x, bf)
    mean = t // N
    one_more = np.concatenate([mean, [total_at(x, bf, WINDOW - N) // N]])       # offset NOFF: samples up to 4095
    return dict(raw_totals=int(np.argmin(t)),
                last_minimum=int(len(mean) - 1 - np.argmin(mean[::-1])),
                rounded_mean=int(np.argmin((t + N // 2) // N)),
                ceiling_mean=int(np.argmin(-(-t // N))),
                one_offset_more=int(np.argmin(one_more)),
                one_offset_fewer=int(np.argmin(mean[:-1])))


WRONG_RULES = ("raw_totals", "last_minimum", "rounded_mean", "ceiling_mean", "one_offset_more", "one_offset_fewer")


# ------------------------------------------------------------------------------------------------ placement checks

def check_model(sw, want):
    """For every stream the model's first-minimum index is the oracle's clock index."""
    assert (want["status"] != I.ST_TOO_SHORT).all()
    for s in range(len(sw.meta)):
        assert first_minimum(window_of(sw, s), int(sw.bf[s])) == int(want["clock_idx"][s]), (int(sw.bf[s]), sw.meta[s])


def check_rate(sw, want, bf):
    """Every placement condition of one rate's streams (``sw`` may hold other rates too)."""
    sel = np.nonzero(sw.bf == bf)[0]
    N, NOFF = 2 * bf, WINDOW - 2 * bf
    ci = want["clock_idx"].astype(np.int64)
    meta = [sw.meta[s] for s in sel]
    assert sorted({m["cls"].replace("_lanes", "").replace("_steps", "").replace("_rt", "") for m in meta}) \
        == classes_of(bf), bf
    assert (sw.ln[sel] >= WINDOW + 2 * N).all()
    assert ((ci[sel] >= 0) & (ci[sel] < NOFF)).all()
    killed = dict.fromkeys(WRONG_RULES, 0)
    answers = {}
    for s in sel:
        answers[s] = wrong_rules(window_of(sw, s), bf)
        for k, v in answers[s].items():
            killed[k] += v != ci[s]
    # every wrong rule answers differently on at least one stream of the rate: families A and B alone refute all six,
    # and they exist at every rate
    assert all(killed[k] > 0 for k in WRONG_RULES), (bf, killed)
    by = lambda **kw: [s for s in sel if all(sw.meta[s].get(k) == v for k, v in kw.items())]  # noqa: E731
    # (A) total(p) sits on the bin edge and one below it, and p wins the stream where it is one below.  The pair
    # separates -- the on-edge stream goes to an EARLIER offset, which the raw-total rule misses -- exactly when some
    # earlier offset does not see the bump: p >= bf / 2 + 1 for the positive bump (offset 0 otherwise covers it at a
    # low position and every offset before p rises a bin), p >= 1 for the negative one
    for sign in (1, -1):
        for p in a_offsets(bf, sign):
            (on,), (past,) = by(fam="A", sign=sign, p=p, v=bf), by(fam="A", sign=sign, p=p, v=bf + 1)
            t_on, t_past = DM.totals(window_of(sw, on), bf), DM.totals(window_of(sw, past), bf)
            assert t_on[p] == 32767 * N and t_past[p] == 32767 * N - 1
            assert ci[past] == p
            if p >= (bf // 2 + 1 if sign > 0 else 1):
                assert ci[on] < p and answers[on]["raw_totals"] == p, (bf, sign, p)
            else:
                assert ci[on] == p, (bf, sign, p)
    assert any(p >= 1 for p in a_offsets(bf, -1))
    # (B) a single pocket inside the search wins where it lies; outside it, the answer stays inside
    inside = by(cls="B1")
    assert ci[inside].tolist() == [sw.meta[s]["p"] for s in inside]
    assert sorted({sw.meta[s]["p"] for s in inside}) == placements(bf)
    for d in (0, 5):
        assert sorted(sw.meta[s]["p"] for s in by(cls="B1", d=d)) == placements(bf)
    outside = by(cls="B_outside")
    assert sorted({sw.meta[s]["p"] for s in outside}) == [NOFF, NOFF + 1] and (ci[outside] < NOFF).all()
    assert all(answers[s]["one_offset_more"] == NOFF for s in by(cls="B_outside", p=NOFF))
    winners = ci[inside]
    assert set((winners & 1).tolist()) == {0, 1}, bf
    for s in seams(bf):
        assert all((s + e in winners) == (0 <= s + e < NOFF) for e in (-1, 0, 1)), (bf, s)
    if form(bf) == "lanes":
        gc = gc_of("lanes")
        lanes = -(-NOFF // gc)
        owner = set((winners // gc).tolist())
        assert {0, lanes - 1} <= owner and any(0 < l < lanes - 1 for l in owner), (bf, owner)
    # (B) two pockets: the oracle picks the intended one, both totals are what the pair was built from
    pairs = by(fam="B2")
    assert ci[pairs].tolist() == [sw.meta[s]["win"] for s in pairs], bf
    for s in pairs:
        m = sw.meta[s]
        t = DM.totals(window_of(sw, s), bf)
        d1, d2 = int(t[m["p1"]]), int(t[m["p2"]])
        assert (d1, d2) == {"same_bin_later_smaller": (N + 3, N), "next_bin_later": (N, N - 1),
                            "same_bin_far": (2 * N - 1, N)}[m["pair"]]
        if m["cls"].startswith("B2_lane"):
            gc = gc_of(m["cls"].rsplit("_", 1)[1])
            assert m["p1"] // gc == m["p2"] // gc
        if m["cls"] == "B2_step":
            step, gc = source_constants()["step"], source_constants()["rt_gc"]
            assert m["p2"] - m["p1"] == step and (m["p1"] % step) // gc == (m["p2"] % step) // gc
    # (C) the winner moves from cycle to cycle as built, and the payload decodes from the moved index
    cs = by(fam="C")
    assert ci[cs].tolist() == [sw.meta[s]["win"] for s in cs], bf
    if cs:
        assert (want["status"][cs] == I.ST_OK).all() and (want["nbytes"][cs] == 2).all(), bf
        assert (want["nbits"][cs] == 28).all()
        assert {sw.meta[s]["variant"] for s in cs} == {v[0] for v in C_VARIANTS}
        assert len({int(c) for c in ci[cs]}) >= 4 and {int(c) & 1 for c in ci[cs]} == {0, 1}
        for s in cs:
            t = DM.totals(window_of(sw, s), bf)
            assert int(t[ci[s]]) // N in (12767 - 1, 12767), (bf, sw.meta[s])
    # (D) aligned offsets of the inverted tiling reach the largest mean there is; the pocket wins
    ds = by(fam="D")
    assert len(ds) == 3
    for s in ds:
        m = sw.meta[s]
        t = DM.totals(window_of(sw, s), bf)
        if m["p"] >= 0:
            assert ci[s] == m["p"] and int(t[m["p"]]) == 5
        elif m["phase"] % N < NOFF:
            assert int(t[m["phase"] % N]) == 65535 * N == int(t.max())
    return killed


def check_all(sw, want):
    check_model(sw, want)
    for bf in sorted(set(sw.bf.tolist())):
        check_rate(sw, want, int(bf))


# ------------------------------------------------------------------------------------------------ live rows

LIVE_RATES = (40, 100)
LIVE_PAYLOAD = 40                   # bytes: the burst outlasts the sync window and several gate blocks
# per-row gate and squelch thresholds, all below family C's level (a block of the burst holds at most 73 lead zeros:
# its mean amplitude stays above 19200)
LIVE_PAIRS = ((18000, 14000), (19200, 19000))


@functools.lru_cache(maxsize=None)
def live_set():
    """Family C at bit_frames 40 and 100 as rows of a ``live_sweep_inputs.LiveSet``: the burst starts on a gate block,
    the lead is inside it.  Families A and B rest on silence and cannot open a gate, family D never falls quiet: they
    have no live rows."""
    from tests import live_sweep_inputs as L
    rows = []
    for bf in LIVE_RATES:
        for x, m in family_c(bf, np.random.default_rng(7100 + bf), LIVE_PAYLOAD):
            x = x[: int(np.nonzero(x)[0][-1]) + 1 + 12 * bf]
            rows.append((x, bf, LIVE_PAIRS[len(rows) % 2][1], dict(m, nbytes=LIVE_PAYLOAD)))
    ls = L.assemble(rows)
    ls.a_start[:] = [LIVE_PAIRS[c % 2][0] for c in range(ls.n)]
    return ls


def check_live(ls, want):
    """One burst per row at block QUIET (``geometry`` asserts it); its clock index is the cycle family C built the
    row for, and the payload decodes from there."""
    from tests import live_sweep_inputs as L
    geo = L.geometry(ls, want)
    assert geo.ci.tolist() == ls.col("win").tolist()
    assert all(w[0]["status"] == I.ST_OK and w[0]["nbytes"] == LIVE_PAYLOAD for w in want)
    assert (ls.a_start < LEVEL).all() and (ls.a_end < LEVEL).all()
    assert len(set(zip(ls.a_start.tolist(), ls.a_end.tolist()))) == 2
    for bf in LIVE_RATES:
        sel = ls.bf == bf
        assert {m["variant"] for m, k in zip(ls.meta, sel) if k} == {v[0] for v in C_VARIANTS}
        assert len(set(geo.ci[sel].tolist())) >= 4 and set((geo.ci[sel] & 1).tolist()) == {0, 1}
    return geo
