"""Input sets of the auto receiver's rate-decision sweeps (tests/test_gpu_auto_sweeps.py) and the placement conditions
each set was built for.  Not a test module.

``LiveAutoSinkT::rate_score`` (afsk_live_auto.hip) scores a candidate in ONE signed pass over the window samples
[ci, ci + n 2bf), a lane taking every 64th sample and stepping its phase by 64 mod 2bf, then divides once; ``decide``
takes the minimum of (score << 6) | list position and packs the winner as (score << 11) | bit_frames.  Clean
transmissions give small scores with equal cycle totals and never tie, so these sets put the decision where that
arithmetic decides something.  Write N = 2 bf, NOFF = 4096 - N, n(ci) = (4095 - N - ci) // N + 1.

  (S) every candidate alone (``candidates=[bf]``, all 36 rates): transmissions at the rate, at half and at twice its
      symbol length, clean and at 5 dB; Gaussian noise at two levels; full-scale random signs; a DC offset under a
      tone; a full-scale tile behind a lead of -32768; the inverted full-scale tile (totals of 65535 N).
  (E) the score's bin edge: the training cycle tiled at level 20000 -- every aligned cycle totals N 12767 + bf, cycle 0
      is the first minimum -- with the phase-0 sample of the last counted cycle lowered by bf n - 1 (score 12767) and by
      bf n (12768).  d(ci) is 12767 in both.  With ``[bf]`` and with all 36 candidates, and with max_score = 12767.
  (N) the cycle count: a lead of constant 20000 in front of the tile moves ci to the lead; the lead takes 0, 1, NOFF - 1
      and both sides of every offset where n drops.  The last counted cycle carries a dent of bf n, the first uncounted
      one a dent of 3 bf (n + 1); every window has a twin that differs from sample 4096 on (silence / full scale).
  (T) ties: constant 20000 with ONE sample lowered by delta.  A candidate scores 32766 where delta > bf n(ci) at its
      own clock index and 32767 otherwise.  Alone at delta = bf and bf + 1; neighbouring pairs in both list orders at
      delta = a + 1 (a alone is lower: it wins from position 1) and b + 1 (a tie: position 0 wins); all 36 descending.
  (P) the rows of largest score and largest bit_frames, for pushes of seeded sizes.

A row is one channel of an ``AutoSet``: ``QUIET`` quiet blocks, the burst from a block boundary on, quiet blocks.
Every expected value is tests/live_auto_model.py's (the oracle's gate, tests/detect_model.py, the oracle's demod); the
``check_*`` functions assert every placement from those outputs, and ``kernel_score`` restates the device's one-pass
form with seven wrong variants for tests/test_auto_sweep_inputs_host.py to refute."""
import functools
from dataclasses import dataclass

import numpy as np

from afskmodem_amd import _native
from tests import detect_model as D
from tests import live_auto_model as M
from tests import symbol_streams as G

WINDOW = 4096
B = 2048                            # the gate's block
QUIET = 2                           # quiet blocks in front of every burst (the gate discards block 0)
LEVEL = 20000                       # above the default gate pair, far below full scale
PAIR = (18000, 14000)               # the default gate and squelch thresholds
PAIRS = ((18000, 14000), (19200, 19000))    # the per-channel cell: both below LEVEL
LOUD = 5                            # loud blocks of a burst at the most: captures of ten blocks
RATES = tuple(D.VALID_BIT_FRAMES)
T_POS, T_POS_FAST = 4000, 4094      # family T's lowered sample: n = 1 there from bit_frames 48 on / at every rate
FAMILIES = ("S", "E", "N", "T")
MAX_SCORE = 12767                   # family E's limit: the first burst of each pair sits on it, the second one above


def n_of(bf, ci):
    """Whole cycles the score counts from clock index ci."""
    return (WINDOW - 2 * bf - 1 - ci) // (2 * bf) + 1


def expected_missing():
    """{family: rates} that geometry rules out, from the inequalities alone.  E and N need two counted cycles at
    ci = 0; T needs a sample position p <= 4094 whose first covering offset p - N + 1 counts one cycle."""
    out = {"E": [], "N": [], "T": []}
    for bf in RATES:
        N = 2 * bf
        if n_of(bf, 0) < 2:
            out["E"].append(bf)
            out["N"].append(bf)
        if not any(p - N + 1 >= 0 and n_of(bf, p - N + 1) == 1 for p in (T_POS, T_POS_FAST)):
            out["T"].append(bf)
    return {k: tuple(v) for k, v in out.items()}


# With N > 2047 a window holds one counted cycle at every clock index: score = d(ci) by definition, family S covers
# those rates.  Family T exists everywhere: position 4094 is covered first by offset NOFF - 1, which counts one cycle.
MISSING = {"E": (1200, 1500, 1600, 1920, 2000), "N": (1200, 1500, 1600, 1920, 2000), "T": ()}


def families_of(bf):
    return tuple(f for f in FAMILIES if bf not in MISSING.get(f, ()))


def t_pos(bf):
    """Family T's sample position for the rate alone: 4000 where one cycle is counted from there, else 4094."""
    return T_POS if n_of(bf, T_POS - 2 * bf + 1) == 1 else T_POS_FAST


# ------------------------------------------------------------------------------------------------ sets of rows

@dataclass
class AutoSet:
    host: np.ndarray                # int16 [n, total]: one channel per row
    candidates: tuple               # the receiver's list (None: all 36)
    meta: list                      # [n] dicts: what the generator intended (grouping only, never an expected value)

    @property
    def n(self):
        return self.host.shape[0]

    def window(self, c):
        return self.host[c, QUIET * B: QUIET * B + WINDOW]

    def burst(self, c):
        """The channel from the burst's first sample to the capture's end (silence behind the burst)."""
        return self.host[c, QUIET * B:]

    def rows(self, **kw):
        return [c for c, m in enumerate(self.meta) if all(m.get(k) == v for k, v in kw.items())]


def assemble(rows, candidates):
    """rows: (burst samples, meta).  The capture ends with a closing block and QUIET quiet ones."""
    blocks = max(-(-len(x) // B) for x, _ in rows)
    assert 2 <= blocks <= LOUD
    host = np.zeros((len(rows), (QUIET + blocks + 1 + QUIET) * B), np.int16)
    for c, (x, _) in enumerate(rows):
        assert x.dtype == np.int16 and len(x) >= WINDOW
        host[c, QUIET * B: QUIET * B + len(x)] = x
    host.setflags(write=False)
    return AutoSet(host, None if candidates is None else tuple(candidates), [m for _, m in rows])


def subset(aset, idx, candidates="same"):
    idx = np.asarray(idx, np.int64)
    return AutoSet(aset.host[idx], aset.candidates if candidates == "same" else candidates,
                   [aset.meta[i] for i in idx])


def concat(sets, candidates):
    total = max(s.host.shape[1] for s in sets)
    host = np.zeros((sum(s.n for s in sets), total), np.int16)
    r = 0
    for s in sets:
        host[r: r + s.n, : s.host.shape[1]] = s.host
        r += s.n
    return AutoSet(host, candidates, [m for s in sets for m in s.meta])


def expected(aset, max_score=None, pairs=None):
    """Per channel the bursts tests/live_auto_model.py expects; ``pairs``: a (start, end) pair per channel."""
    return [M.expected(aset.host[c], aset.candidates, max_score, *(pairs[c] if pairs else PAIR))
            for c in range(aset.n)]


def check_gate(aset, want):
    """From the oracle's gate: one burst per channel, from block QUIET on, at least the window long, closed by a
    quiet block -- so the window the builder crafted is the burst's first 4096 samples."""
    for c, w in enumerate(want):
        assert len(w) == 1 and w[0]["start"] == QUIET * B and w[0]["len"] >= WINDOW and w[0]["flags"] == 0, \
            (aset.meta[c], [(b["start"], b["len"], b["flags"]) for b in w])
        assert not aset.host[c, : QUIET * B].any()


def detected(aset, want, c):
    """(bit_frames, rate_score, clock_idx) of channel c's burst, from the expected rows."""
    w = want[c][0]
    return w["bit_frames"], w["rate_score"], w["clock_idx"]


# ------------------------------------------------------------------------------------------------ the generators

def cycle(bf, level=None):
    tc = D.training_cycle(bf)
    return tc if level is None else np.sign(tc) * level


def square(L, bits):
    """Symbols of L samples at full scale: a mark has two periods, a space one.  The oracle's tones where L is a
    rate's symbol length (tests/test_auto_sweep_inputs_host.py); any L >= 2 otherwise."""
    i = np.arange(L)
    mark = np.where((4 * i // L) % 2 == 0, D.HI, D.LO)
    space = np.where((2 * i // L) % 2 == 0, D.HI, D.LO)
    return np.stack([space, mark])[np.asarray(bits, np.int64)].reshape(-1)


def cut(x):
    """At most LOUD blocks, as int16."""
    return np.asarray(x[: LOUD * B]).astype(np.int16)


def tile_stream(bf, lead=0, dents=None, payload=None):
    """``lead`` samples of constant LEVEL, then training cycles at LEVEL past the window's end (cycle k's phase-0 sample
    lowered by dents[k]) -- and, where that fits LOUD blocks, the terminator and a coded payload."""
    N = 2 * bf
    ncyc = -(-(WINDOW + N - lead) // N)
    bits = [1, 0] * ncyc
    if payload is not None and lead + (len(bits) + 4 + 14 * len(payload) + 1) * bf <= LOUD * B:
        bits = G.training(ncyc) + G.coded(payload)
    level = {k: (LEVEL, 0) for k in range(len(bits))}
    for k, d in (dents or {}).items():
        assert 0 <= k < ncyc and 0 < d <= LEVEL
        level[2 * k] = (LEVEL, -d)
    return np.concatenate([np.full(lead, LEVEL, np.int16), G.render(bits, bf, level)])


def family_s(bf, rng):
    N = 2 * bf
    rows = []
    bits = lambda L: [1, 0] * (-(-(WINDOW + 2 * B) // (2 * L)) + 1) + [1, 0, 0, 0] + G.coded(b"auto")  # noqa: E731
    for name, L in (("same", bf), ("half", bf // 2), ("twice", 2 * bf)):
        for snr in (None, 5.0):
            for lead in (0, int(rng.integers(1, 800))):
                x = np.concatenate([np.zeros(lead, np.int64), square(L, bits(L))])
                rows.append((D.add_noise(cut(x), snr, rng), dict(kind="tx_" + name, snr=snr or 0, lead=lead)))
    for sigma in (32000.0, 64000.0):
        for _ in range(2):
            x = np.clip(np.rint(rng.normal(0.0, sigma, WINDOW + B)), D.LO, D.HI)
            rows.append((cut(x), dict(kind="noise", sigma=int(sigma))))
    for _ in range(2):
        rows.append((cut((rng.integers(0, 2, WINDOW + B) * 2 - 1) * D.HI), dict(kind="signs")))
    tone = cycle(bf, LEVEL)[np.arange(WINDOW + B) % N]
    for dc in (6000, -6000):
        rows.append((cut(tone + dc), dict(kind="dc", dc=dc)))
    full = cycle(bf)[np.arange(WINDOW + B) % N]
    rows.append((cut(np.concatenate([np.full(3, D.LO), full])), dict(kind="lowest")))
    inv = ~cycle(bf)
    for phase in (0, 5):
        rows.append((cut(inv[(np.arange(WINDOW + B) - phase) % N]), dict(kind="inverted", phase=phase)))
    return [(x, dict(m, fam="S", bf=bf)) for x, m in rows]


def family_e(bf, rng):
    n = n_of(bf, 0)
    assert n >= 2
    payload = bytes(rng.integers(0, 256, 2, dtype=np.uint8))
    return [(cut(tile_stream(bf, 0, {n - 1: e}, payload)), dict(fam="E", bf=bf, e=e, n=n, side=side))
            for side, e in (("on", bf * n - 1), ("past", bf * n))]


def n_leads(bf):
    """0, 1, NOFF - 1 and both sides of every offset at which the count drops."""
    N, NOFF = 2 * bf, WINDOW - 2 * bf
    drops = [c for c in range(NOFF) if (WINDOW - 1 - N - c) % N == 0]
    return sorted({0, 1, NOFF - 1} | {c + e for c in drops for e in (0, 1) if c + e < NOFF})


def family_n(bf):
    N = 2 * bf
    rows = []
    for lead in n_leads(bf):
        n = n_of(bf, lead)
        inside = tile_stream(bf, lead, {n - 1: bf * n, n: 3 * bf * (n + 1)})[:WINDOW]
        assert lead + n * N < WINDOW                           # the uncounted cycle's dent lies inside the window
        for twin, tail in (("silence", np.zeros(0, np.int16)), ("full", np.full(B, D.HI, np.int16))):
            rows.append((np.concatenate([inside, tail]), dict(fam="N", bf=bf, lead=lead, n=n, twin=twin)))
    return rows


def dented(p, delta):
    x = np.full(WINDOW + B, LEVEL, np.int16)
    x[p] -= delta
    return x


def family_t(bf):
    p = t_pos(bf)
    return [(dented(p, d), dict(fam="T", bf=bf, p=p, delta=d)) for d in (bf, bf + 1)]


def rows_alone(bf):
    """Rows of ``rate_set(bf)``: family S, two of T, and where they exist two of E and a twin pair per lead of N."""
    return sum(S_KINDS.values()) + 2 + (2 + 2 * len(n_leads(bf)) if "E" in families_of(bf) else 0)


@functools.lru_cache(maxsize=4)
def rate_set(bf):
    """Every row of one rate for the receiver with ``candidates=[bf]``."""
    rng = np.random.default_rng(9000 + bf)
    rows = family_s(bf, rng)
    if "E" in families_of(bf):
        rows += family_e(bf, rng) + family_n(bf)
    rows += family_t(bf)
    return assemble(rows, [bf])


@functools.lru_cache(maxsize=None)
def full_list_e():
    """Family E of every rate that has it, for the receiver with all 36 candidates."""
    rows = []
    for bf in RATES:
        if "E" in families_of(bf):
            rows += family_e(bf, np.random.default_rng(9000 + bf))
    return assemble(rows, None)


def t_pairs():
    """Neighbouring rates (a, b, p): from 48 on at position 4000, the eight faster ones at 4094."""
    slow = [bf for bf in RATES if t_pos(bf) == T_POS]
    fast = [bf for bf in RATES if t_pos(bf) != T_POS]
    return [(a, b, T_POS) for a, b in zip(slow, slow[1:])] + [(a, b, T_POS_FAST) for a, b in zip(fast, fast[1:])]


def pair_set(a, b, p, order):
    """The list ``order`` of (a, b): no candidate lower, a alone lower, both lower."""
    rows = [(dented(p, d), dict(fam="T", a=a, b=b, p=p, delta=d)) for d in (a, a + 1, b + 1)]
    return assemble(rows, order)


DESCENDING = tuple(sorted(RATES, reverse=True))
DESCENDING_DELTAS = (48, 49, 61, 101, 129)     # at most 3 * 48: every lowered candidate is ONE bin lower


@functools.lru_cache(maxsize=None)
def descending_set():
    return assemble([(dented(T_POS, d), dict(fam="T", p=T_POS, delta=d)) for d in DESCENDING_DELTAS], DESCENDING)


# ------------------------------------------------------------------------------------------------ the device's form

FORMS = ("n_more", "n_fewer", "rounded", "d_ci", "space_two", "quarter_shift")
N_FORMS = ("n_fewer", "d_ci")       # refuted only where more than one cycle is counted: families E and N


def kernel_score(x, bf, ci, form=None):
    """``rate_score`` as the device computes it: lane l takes samples l, l + 64, ... of [ci, ci + n N) at the phases
    ``lane_phases`` restates, the three-range test gives the sign, the signed sum is subtracted from 65535 bf n in
    uint32 and divided once, truncating.  ``x``: the burst (the window first; what lies behind it is only ever read by
    the wrong form with one cycle too many).  ``form``: one of FORMS, the defect to build in."""
    N, q = 2 * bf, bf >> 2
    n = n_of(bf, ci)
    n = {"n_more": n + 1, "n_fewer": max(n - 1, 1), "d_ci": 1}.get(form, n)
    total = n * N
    x = np.asarray(x[ci: ci + total], np.int64)
    if total > len(x):
        x = np.concatenate([x, np.zeros(total - len(x), np.int64)])
    p = lane_phases(bf, total)
    if form == "quarter_shift":
        p = (p + q) % N
    high = (p < q) | ((p >= 2 * q) & (p < 3 * q)) | ((p >= bf) & (p < bf + 2 * q))
    if form == "space_two":
        high = (p < q) | ((p >= 2 * q) & (p < 3 * q)) | ((p >= bf) & (p < bf + q)) | ((p >= bf + 2 * q) & (p < bf + 3 * q))
    s = int(np.where(high, x, -x).sum())
    assert abs(s) < (1 << 27 if form is None else 1 << 31)
    num = (65535 * bf * n - s) & 0xFFFFFFFF
    return (num + total // 2) // total if form == "rounded" else num // total


def lane_phases_stepped(bf, total):
    """The phase of every sample j < total as the lanes step it: lane l starts at l mod N and adds 64 mod N per step,
    subtracting N once when it reaches it."""
    N = 2 * bf
    inc = 64 % N
    out = np.empty(total, np.int64)
    for lane in range(min(64, total)):
        ph = lane % N
        for j in range(lane, total, 64):
            out[j] = ph
            ph += inc
            if ph >= N:
                ph -= N
    return out


def lane_phases(bf, total):
    """``lane_phases_stepped`` in closed form (the CPU suite holds the two together at every rate)."""
    j = np.arange(total)
    return (j % 64 % (2 * bf) + (j // 64) * (64 % (2 * bf))) % (2 * bf)


def decide(scores, last_wins=False):
    """The list position ``decide`` picks: the minimum of (score << 6) | position -- or, the defect, of the key with
    the positions counted from the list's end."""
    k = len(scores)
    keys = [(int(s) << 6) | ((k - 1 - p) if last_wins else p) for p, s in enumerate(scores)]
    return int(np.argmin(keys))


def check_forms(aset, killed=None):
    """For every row of a one-candidate set: the device's form equals the model's score, and each wrong form is
    counted where it differs.  Returns {form: count}."""
    (bf,) = aset.candidates
    killed = killed if killed is not None else dict.fromkeys(FORMS, 0)
    for c in range(aset.n):
        score, ci, _ = D.candidate(aset.window(c), bf)
        assert kernel_score(aset.burst(c), bf, ci) == score, (bf, aset.meta[c])
        for f in FORMS:
            killed[f] += kernel_score(aset.burst(c), bf, ci, f) != score
    return killed


# ------------------------------------------------------------------------------------------------ placement checks

S_KINDS = {"tx_same": 4, "tx_half": 4, "tx_twice": 4, "noise": 4, "signs": 2, "dc": 2, "lowest": 1, "inverted": 2}


def check_rate(aset, want):
    """Every placement of one rate's rows, from the expected rows and the model."""
    (bf,) = aset.candidates
    N, NOFF = 2 * bf, WINDOW - 2 * bf
    check_gate(aset, want)
    assert tuple(sorted({m["fam"] for m in aset.meta}, key=FAMILIES.index)) == families_of(bf)
    for c in range(aset.n):
        got = detected(aset, want, c)
        score, ci, _ = D.candidate(aset.window(c), bf)
        assert got == (bf, score, ci), (bf, aset.meta[c], got)
    # (S) every kind is there; the inverted tile's aligned offsets reach the largest total and -32768 is in a window
    kinds = [aset.meta[c]["kind"] for c in aset.rows(fam="S")]
    assert {k: kinds.count(k) for k in S_KINDS} == S_KINDS and len(kinds) == sum(S_KINDS.values())
    (top,) = aset.rows(fam="S", kind="inverted", phase=0)
    assert int(D.totals(aset.window(top), bf).max()) == 65535 * N
    (low,) = aset.rows(fam="S", kind="lowest")
    assert (aset.window(low) == D.LO).any() and (aset.window(low)[:3] == D.LO).all()
    # (E) both rows at clock index 0 with d(0) = 12767, n >= 2 cycles counted, the score on and past the bin edge
    if "E" in families_of(bf):
        (on,), (past,) = aset.rows(fam="E", side="on"), aset.rows(fam="E", side="past")
        n = n_of(bf, 0)
        assert n >= 2 and aset.meta[on]["n"] == n
        for c, s in ((on, 12767), (past, 12768)):
            assert D.candidate(aset.window(c), bf) == (s, 0, 12767), (bf, aset.meta[c])
            t = D.totals(aset.window(c), bf)
            assert int(t[0]) == N * 12767 + bf and int(t[(n - 1) * N]) == N * 12767 + bf + aset.meta[c]["e"]
        assert (aset.meta[on]["e"], aset.meta[past]["e"]) == (bf * n - 1, bf * n)
    else:
        assert n_of(bf, 0) == 1 and not aset.rows(fam="E")
    # (N) ci = the lead at every lead, n as the definition has it and dropping by one across every listed offset; the
    # last counted and the first uncounted cycle differ; the twins share the window and differ behind it
    if "N" in families_of(bf):
        leads = n_leads(bf)
        assert {0, 1, NOFF - 1} <= set(leads)
        drops = [c for c in range(NOFF) if (WINDOW - 1 - N - c) % N == 0]
        assert len(drops) == n_of(bf, 0) and all(c in leads and (c + 1 in leads or c + 1 == NOFF) for c in drops)
        for c0 in drops[:-1]:
            assert n_of(bf, c0) == n_of(bf, c0 + 1) + 1
        for lead in leads:
            a, b = aset.rows(fam="N", lead=lead, twin="silence"), aset.rows(fam="N", lead=lead, twin="full")
            assert len(a) == 1 and len(b) == 1
            a, b = a[0], b[0]
            n = n_of(bf, lead)
            assert detected(aset, want, a) == detected(aset, want, b) == (bf, 12768, lead), (bf, lead)
            assert np.array_equal(aset.window(a), aset.window(b))
            assert not aset.burst(a)[WINDOW: WINDOW + B].any() and (aset.burst(b)[WINDOW: WINDOW + B] == D.HI).all()
            w = aset.window(a).astype(np.int64)
            assert LEVEL - w[lead + (n - 1) * N] == bf * n and LEVEL - w[lead + n * N] == 3 * bf * (n + 1)
            assert lead + (n + 1) * N - 1 >= WINDOW - 1        # the uncounted cycle ends at or behind sample 4095
    else:
        assert not aset.rows(fam="N")
    # (T) delta = bf ties with everything (32767 at clock index 0), bf + 1 is one bin lower where ONE cycle is counted
    (on,), (past,) = aset.rows(fam="T", delta=bf), aset.rows(fam="T", delta=bf + 1)
    p = aset.meta[on]["p"]
    assert detected(aset, want, on) == (bf, 32767, 0)
    assert detected(aset, want, past) == (bf, 32766, p - N + 1) and n_of(bf, p - N + 1) == 1


def check_full_list_e(aset, want, refused=None):
    """All 36 candidates name the tile's rate at clock index 0, the runner-up far away; scores 12767 and 12768."""
    check_gate(aset, want)
    assert aset.candidates is None and sorted({m["bf"] for m in aset.meta}) == [b for b in RATES if b not in MISSING["E"]]
    for c, m in enumerate(aset.meta):
        det = D.detect(aset.window(c))
        assert (det["bit_frames"], det["score"], det["clock_idx"]) == (m["bf"], 12767 + (m["side"] == "past"), 0), m
        assert det["runner_up"] >= det["score"] + 1000, (m, det["runner_up"])
        assert detected(aset, want, c) == (m["bf"], det["score"], 0)
        if refused is not None:
            r = refused[c][0]
            if m["side"] == "on":
                assert r == want[c][0] and r["status"] != _native.ST_INVALID_BAUD
            else:
                assert (r["status"], r["bit_frames"], r["rate_score"], r["clock_idx"], r["term_frame"], r["nbytes"],
                        r["nbits"], r["bytes"]) == (_native.ST_INVALID_BAUD, 0, 12768, -1, -1, 0, 0, b"")


def check_pair(aset, want):
    """The three rows of one pair list: a tie of the whole list at 32767, a alone lower, both lower."""
    check_gate(aset, want)
    a, b = sorted(aset.candidates)
    first = aset.candidates[0]
    got = [detected(aset, want, c)[:2] for c in range(3)]
    assert [m["delta"] for m in aset.meta] == [a, a + 1, b + 1]
    assert got == [(first, 32767), (a, 32766), (first, 32766)], (aset.candidates, got)
    scores = [D.detect(aset.window(c), aset.candidates)["scores"] for c in range(3)]
    assert scores[0] == [32767, 32767] and scores[2] == [32766, 32766]
    assert scores[1] == ([32767, 32766] if first == b else [32766, 32767])
    return scores


def check_descending(aset, want):
    """All 36 in descending order: a candidate is one bin lower where bf n < delta at its own clock index; the winner
    is the largest of them, deep in the list, with the others tied behind it; delta = 48 lowers nobody and position 0
    wins."""
    check_gate(aset, want)
    deep = 0
    for c, m in enumerate(aset.meta):
        det = D.detect(aset.window(c), aset.candidates)
        lower = [bf for bf in aset.candidates if bf * n_of(bf, T_POS - 2 * bf + 1) < m["delta"]]
        assert [bf for bf, s in zip(aset.candidates, det["scores"]) if s == 32766] == lower, m
        assert all(s in (32766, 32767) for s in det["scores"])
        win = lower[0] if lower else aset.candidates[0]
        assert detected(aset, want, c)[:2] == (win, 32766 if lower else 32767), m
        deep += bool(lower) and aset.candidates.index(win) >= 8 and len(lower) >= 2
    assert deep >= 2


# ------------------------------------------------------------------------------------------------ reduced rows, P

CELL_RATES = (40, 1000)             # the two forms of the sink's clock search: bit_frames 40, and the run-time form at
                                    # the largest rate that has every family


def reduced(bf, want):
    """One row per family of the rate: the family's row of largest expected score, the first of them on a tie."""
    aset = rate_set(bf)
    assert families_of(bf) == FAMILIES
    return [max(aset.rows(fam=f), key=lambda c: (want[c][0]["rate_score"], -c)) for f in FAMILIES]


def cell_sets():
    """The reduced rows for the tapped, the ragged and the per-channel cells: per form its rate's list, and both
    rates' rows under all 36 candidates."""
    parts = []
    for bf in CELL_RATES:
        aset = rate_set(bf)
        parts.append(subset(aset, reduced(bf, expected(aset))))
    return parts + [concat(parts, None)]


P_STEPS = [1, 7, 2047, 2048, 2049, 8192]
P_TOP = 8


def p_sets():
    """The rows of S and E with the largest scores and the largest bit_frames: family S of rate 2000 alone -- the
    largest rate, every score packed beside it --, and under all 36 candidates the P_TOP rows of largest score and the
    P_TOP of largest bit_frames among the S rows of 40 and 2000 and the E rows of every rate."""
    alone = subset(rate_set(2000), rate_set(2000).rows(fam="S"))
    pool = concat([subset(rate_set(bf), rate_set(bf).rows(fam="S")) for bf in (40, 2000)] + [full_list_e()], None)
    det = [D.detect(pool.window(c)) for c in range(pool.n)]
    by_score = sorted(range(pool.n), key=lambda c: (-det[c]["score"], c))[:P_TOP]
    by_rate = sorted(range(pool.n), key=lambda c: (-det[c]["bit_frames"], c))[:P_TOP]
    return alone, subset(pool, sorted(set(by_score + by_rate)))
