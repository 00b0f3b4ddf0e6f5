"""Input sets of the streaming live receiver's boundary sweeps (tests/test_gpu_live_sweeps.py) and the placement
conditions each set was built for.  Not a test module.

The streaming sink (afsk_live_stream.hip) decodes a burst one 2048-sample gate block at a time and carries the last
three decisions, the ``nbits % 7`` pending coded bits, a high nibble and the uncommitted symbol's samples from block to
block.  These sets put a block edge at every place where one of those carries matters -- inside a symbol at every
residue, inside the terminator, at a squelch stop, inside a codeword at every count of pending bits -- and add symbols
whose mark and space sums are within one ``bit_frames`` of each other, which no full-scale tone ever produces.

A case is a ROW of a ``LiveSet``: ``QUIET`` quiet blocks, the generated stream (tests/symbol_streams.py) from a block
boundary on, its ``lead`` zeros first so that the burst's clock index is the lead, then at least ``QUIET`` quiet blocks
-- or, for the rows that are still loud at the flush, signal up to the row's last sample.  ``expected`` is the oracle's
gate over the whole row and the oracle's demod of every burst it cut; the ``check_*`` functions assert, from those
outputs (and, for the near ties, plain numpy sums of the samples), that the gate cut one burst per row at block
``QUIET`` and that every placement happened, so a drifting generator fails loudly instead of quietly covering less.
tests/test_live_sweep_inputs_host.py runs the checks and the block-by-block model on the CPU; the GPU sweeps run the
checks again on the very rows they compare against."""
import functools
from dataclasses import dataclass

import numpy as np

from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests import split_sweep_inputs as I
from tests import symbol_streams as G

B = 2048                            # the gate's block
QUIET = 3                           # quiet blocks in front of and behind every stream
FIELDS = ("nbytes", "nbits", "clock_idx", "term_frame", "status")
ST_OK, ST_NO_DATA = 0, 2


@dataclass
class LiveSet:
    host: np.ndarray                # int16 [n, total]: one channel per row
    bf: np.ndarray                  # int32 [n]
    a_start: np.ndarray             # int32 [n]
    a_end: np.ndarray               # int32 [n]
    meta: list                      # [n] dicts: what the generator intended (grouping only, never an expected value)

    def col(self, key, default=-1):
        return np.array([m.get(key, default) for m in self.meta], np.int64)

    @property
    def n(self):
        return self.host.shape[0]

    @property
    def maxp(self):
        """Payload bytes per burst that hold every row's whole payload."""
        return int(self.host.shape[1] // (14 * int(self.bf.min()))) + 8


def assemble(closed, still_loud=()):
    """closed: (stream samples, bit_frames, amp_end, meta).  still_loud: (maker, bit_frames, amp_end, meta) with
    maker(L) -> exactly L samples that are loud to the last one: the burst the flush reports."""
    blocks = max(-(-len(x) // B) for x, _, _, _ in closed)
    total = (2 * QUIET + blocks) * B
    rows = list(closed) + [(make(total - QUIET * B), bf, a, m) for make, bf, a, m in still_loud]
    host = np.zeros((len(rows), total), np.int16)
    for c, (x, _, _, _) in enumerate(rows):
        assert len(x) <= total - QUIET * B
        host[c, QUIET * B: QUIET * B + len(x)] = x
    i32 = lambda v: np.array(v, np.int32)  # noqa: E731
    return LiveSet(host, i32([r[1] for r in rows]), i32([18000] * len(rows)), i32([r[2] for r in rows]),
                   [r[3] for r in rows])


def subset(ls, idx):
    idx = np.asarray(idx)
    return LiveSet(ls.host[idx], ls.bf[idx], ls.a_start[idx], ls.a_end[idx], [ls.meta[i] for i in idx])


def concat(sets):
    """Rows of several sets in one, the shorter ones padded with silence."""
    # (a subset may be shorter than the set it was taken from)
    used = [(int(np.nonzero(s.host.any(axis=0))[0][-1]) // B + 1 + QUIET) * B for s in sets]
    assert all(u <= s.host.shape[1] for u, s in zip(used, sets))
    host = np.zeros((sum(s.n for s in sets), max(used)), np.int16)
    r = 0
    for s, u in zip(sets, used):
        host[r: r + s.n, :u] = s.host[:, :u]
        r += s.n
    cat = lambda k: np.concatenate([getattr(s, k) for s in sets])  # noqa: E731
    return LiveSet(host, cat("bf"), cat("a_start"), cat("a_end"), [m for s in sets for m in s.meta])


def expected(ls, rows=None, maxp=None):
    """Per row the bursts the oracle's gate cuts and the oracle's demod of each (tests/test_gpu_live_stream.py's
    ``expected``, with ``corrected``)."""
    maxp = ls.maxp if maxp is None else maxp
    out = []
    for c in range(ls.n) if rows is None else rows:
        cap, bf, a_end = ls.host[c], int(ls.bf[c]), int(ls.a_end[c])
        bursts, oe = O.gate_stream(cap, int(ls.a_start[c]), a_end, 64)
        got = []
        for j, (s, n) in enumerate(bursts):
            r = O.demod_batch_soft(cap[s: s + n], [0], [n], [bf], a_end, out_stride=max(maxp, 1), margin_stride=1)
            row = dict(start=s, len=n, flags=_native.LIVE_OPEN_END if (oe and j == len(bursts) - 1) else 0)
            row.update({f: int(r[f][0]) for f in FIELDS})
            row["corrected"] = int(r["corrected"][0])
            row["bytes"] = r["bytes"][0, : min(row["nbytes"], maxp)].tobytes()
            got.append(row)
        out.append(got)
    return out


@dataclass
class Geometry:
    ln: np.ndarray                  # the burst's length
    ci: np.ndarray                  # clock index
    first: np.ndarray               # first data symbol
    K: np.ndarray                   # symbols with i < len - bf (ref:362, 372)
    nbits: np.ndarray
    open_end: np.ndarray            # bool


def geometry(ls, want):
    """Asserts one burst per row, starting at block QUIET; the burst's geometry from the oracle's outputs."""
    for c, w in enumerate(want):
        assert len(w) == 1 and w[0]["start"] == QUIET * B, (c, [(b["start"], b["len"]) for b in w])
    col = lambda k: np.array([w[0][k] for w in want], np.int64)  # noqa: E731
    ln, ci, tf, bf = col("len"), col("clock_idx"), col("term_frame"), ls.bf.astype(np.int64)
    assert (ci >= 0).all()
    return Geometry(ln, ci, (tf - ci) // bf, (ln - ci - 1) // bf, col("nbits"), col("flags") == _native.LIVE_OPEN_END)


def committed(geo, bf, c, j):
    """Symbols of row c the sink has committed once j blocks are recorded: those with ci + (k + 1) bf < j B."""
    return (j * B - int(geo.ci[c]) - 1) // int(bf[c])


def live_edges(ls, geo, c):
    """The block edges j >= 2 of row c's burst (j blocks recorded) up to the end of the symbol after the last one the
    oracle decoded: the edges at which the sink still has symbols to carry."""
    bf = int(ls.bf[c])
    end = int(geo.ci[c]) + (int(geo.first[c]) + int(geo.nbits[c]) + 1) * bf
    return [j for j in range(2, int(geo.ln[c]) // B + 1) if j * B <= end]


def _payload(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


# --------------------------------------------------------------------------------------------------------- (A)
A_RATES = (8, 40, 100, 160, 2000)
# (j B - lead) % bf over the edges j: B % bf = 0, 8, 48, 128, 48 -- every residue needs leads 0 ... gcd(B, bf) - 1;
# 160: five residues per lead; 2000: 48 j = 2016 at j = 42, so leads 16, 15 and 17 give 0, 1 and bf - 1 there
A_LEADS = {8: tuple(range(8)), 40: tuple(range(8)), 100: tuple(range(4)), 160: (0, 1, 2, 3, 158, 159),
           2000: (16, 15, 17, 0, 47, 95)}
# loud blocks of the rows a quiet block closes (100: 48 j % 100 takes its 25 values over 25 edges)
A_BLOCKS = {8: 9, 40: 9, 100: 28, 160: 10, 2000: 46}


def _a_train(bf):
    return G.training(1 if bf == 2000 else 30)


@functools.lru_cache(maxsize=None)
def set_a():
    rng = np.random.default_rng(5001)
    closed, loud = [], []
    for bf in A_RATES:
        train = _a_train(bf)
        for lead in A_LEADS[bf]:
            nsym = A_BLOCKS[bf] * B // bf
            data = G.coded(_payload(rng, nsym // 14 + 1))[: nsym - len(train)]
            closed.append((G.stream(train, data, bf, lead=lead), bf, 14000, dict(lead=lead)))
    total = (2 * QUIET + max(-(-len(x) // B) for x, _, _, _ in closed)) * B
    L = total - QUIET * B
    for bf in A_RATES:
        # a symbol that ends on the last recorded sample (lead = L % bf), and one that ends a sample before it
        hit = L % bf if L % bf < 4096 - 2 * bf - 1 else 16
        for lead in (hit, hit + 1):
            bits = _a_train(bf) + G.coded(_payload(rng, L // bf // 14 + 2))

            def make(n, bits=bits, bf=bf, lead=lead):
                x = G.render(bits, bf, lead=lead)
                assert len(x) >= n
                return x[:n]
            loud.append((make, bf, 14000, dict(lead=lead, loud=1)))
    ls = assemble(closed, loud)
    assert ls.host.shape[1] == total
    return ls


def check_a(ls, want):
    geo = geometry(ls, want)
    assert geo.ci.tolist() == ls.col("lead").tolist()
    assert (geo.ln >= 8 * B).all()
    assert geo.open_end.tolist() == (ls.col("loud", 0) == 1).tolist() and geo.open_end.any() and (~geo.open_end).any()
    assert all(w[0]["status"] == ST_OK for w in want)
    # a burst still loud at the flush decodes to its last whole symbol
    assert (geo.nbits[geo.open_end] == (geo.K - geo.first)[geo.open_end]).all()
    on_last = (geo.ln - geo.ci) % ls.bf == 0
    assert (~on_last & geo.open_end).any()
    for bf in (8, 40, 100, 160):                                # (2000: only where len % 2000 is a lead the clock finds)
        assert (on_last & geo.open_end & (ls.bf == bf)).any(), bf
    for bf in A_RATES:
        res = set()
        for c in np.nonzero(ls.bf == bf)[0]:
            res |= {(j * B - int(geo.ci[c])) % bf for j in live_edges(ls, geo, c)}
        if bf in (8, 40, 100):
            assert res == set(range(bf)), (bf, sorted(set(range(bf)) - res))
        else:
            assert {0, 1, bf - 1} <= res and len(res) >= 19, (bf, len(res))
    return geo


# --------------------------------------------------------------------------------------------------------- (B)
B_RATES = (40, 8, 100)
B_PAYLOAD = {40: 6, 8: 64, 100: 6}      # bytes behind the terminator (8: enough samples to open the gate and go on)
B_EDGES = (2, 4)                    # the terminator also ends exactly on these edges


def b_last(bf):
    """The terminator's last symbol goes up to the symbol that ends in the sixth block, and a little further."""
    return 6 * B // bf + 4


@functools.lru_cache(maxsize=None)
def set_b():
    """The terminator's last symbol at every index 3, 5, 6, 7 ... (index 4 cannot exist: symbols 0 and 1 of a locked
    clock are the training cycle 1,0, and a terminator ending at 4 has symbol 1 = 1)."""
    rng = np.random.default_rng(5002)
    rows = []
    for bf in B_RATES:
        for i, kt in enumerate([3] + list(range(5, b_last(bf) + 1))):
            x = G.stream(G.training_ending_at(kt), G.coded(_payload(rng, B_PAYLOAD[bf])), bf, lead=i % 6)
            rows.append((x, bf, 14000, dict(lead=i % 6)))
        for j in B_EDGES:
            # ci + (kt + 1) bf == j B: the terminator's last symbol ends on the last recorded sample and waits
            lead = (j * B) % bf
            kt = (j * B - lead) // bf - 1
            x = G.stream(G.training_ending_at(kt), G.coded(_payload(rng, B_PAYLOAD[bf])), bf, lead=lead)
            rows.append((x, bf, 14000, dict(lead=lead, on_edge=j)))
        for i, d in enumerate((-1, 0, 1, 2)):
            # a data-like 1,0,0,0 inside the training, around the edge between blocks 1 and 2: the scan stops there,
            # the rest of the training is data
            kt = 2 * B // bf + d
            rest = [1, 0] * 20 + [1, 0, 0, 0]
            x = G.stream(G.training_ending_at(kt) + rest, G.coded(_payload(rng, B_PAYLOAD[bf])), bf, lead=i)
            rows.append((x, bf, 14000, dict(lead=i, false=1)))
    return assemble(rows)


def check_b(ls, want):
    geo = geometry(ls, want)
    kt = geo.first - 1
    assert geo.ci.tolist() == ls.col("lead").tolist()
    assert all(w[0]["status"] == ST_OK for w in want)
    false = ls.col("false", 0) == 1
    data = 14 * np.array([B_PAYLOAD[int(f)] for f in ls.bf])
    assert (geo.nbits == data + np.where(false, 44, 0)).all()
    for bf in B_RATES:
        sel = (ls.bf == bf) & ~false
        assert set(kt[sel].tolist()) == {3} | set(range(5, b_last(bf) + 1)), bf
        assert set((kt[sel] & 1).tolist()) == {0, 1}
        assert false[ls.bf == bf].sum() == 4
        # the four symbols decided in one go when the clock locks; ending in the sixth block
        assert (geo.ci[sel] + (kt[sel] + 1) * bf < 2 * B).any() and (geo.ci[sel] + (kt[sel] + 1) * bf > 5 * B).any()
        splits, on_edge = {}, set()
        for c in np.nonzero(ls.bf == bf)[0]:
            end = int(geo.ci[c]) + (int(kt[c]) + 1) * bf
            if end % B == 0:
                on_edge.add(end // B)
            for j in range(2, 6):
                done = min(max(committed(geo, ls.bf, c, j) - (int(kt[c]) - 3), 0), 4)   # of the terminator's four
                if 0 < done < 4:
                    splits.setdefault(j, set()).add(done)
        assert splits[2] == {1, 2, 3} and any(splits[j] == {1, 2, 3} for j in (3, 4, 5)), (bf, splits)
        assert set(B_EDGES) <= on_edge, (bf, on_edge)
    return geo


# --------------------------------------------------------------------------------------------------------- (C)
C_AMP_ENDS = I.D_AMP_ENDS


@functools.lru_cache(maxsize=None)
def set_c(far):
    """The whole-signal cases of ``split_sweep_inputs.sweep_d`` at both squelch thresholds, each row gated and
    squelched with its own pair: the first dimmed data symbol at 0 ... 140 (``far``: around symbol 4096 instead),
    silent, one below the threshold, and exactly on it."""
    rows = []
    for amp_end in C_AMP_ENDS:
        sw = I.sweep_d(amp_end)
        for s, m in enumerate(sw.meta):
            if m.get("end") or bool(m.get("far")) != bool(far):
                continue
            x = sw.flat[int(sw.off[s]): int(sw.off[s]) + int(sw.ln[s])]
            rows.append((x, int(sw.bf[s]), amp_end, dict(variant=m["variant"], far=int(far))))
        if not far:
            # bit_frames 8: symbols 44 ... 184 all end inside block 0, so the same three variants once more around
            # symbol 512, where block 2 begins
            data = G.coded(_payload(np.random.default_rng(5003), 48))
            for i, k in enumerate(range(2 * B // 8 - 3, 2 * B // 8 + 4)):
                for variant in range(3):
                    level, _ = I._dimmed(k - len(I.D_TRAIN), variant, amp_end)
                    x = G.stream(I.D_TRAIN, data, 8, lead=i % 4, level=level)
                    rows.append((x, 8, amp_end, dict(variant=variant, far=0, extra=1)))
    return assemble(rows)


def check_c(ls, want, far):
    geo = geometry(ls, want)
    assert (geo.first == len(I.D_TRAIN)).all()
    variant = ls.col("variant")
    status = np.array([w[0]["status"] for w in want])
    assert (status == np.where(geo.nbits == 0, ST_NO_DATA, ST_OK)).all()
    # the dimmed symbol, from the oracle's stop: on the threshold it does not stop, a silent one D_LATER on does
    dim = geo.nbits - np.where(variant == 2, I.D_LATER, 0)
    assert (dim >= 0).all()
    stops = geo.first + dim
    for bf in (I.RATES if not far else (40, 8)):
        for amp_end in C_AMP_ENDS:
            for v in range(3):
                sel = (ls.bf == bf) & (ls.a_end == amp_end) & (variant == v) & (ls.col("extra", 0) == 0)
                if not far:
                    assert sorted(dim[sel].tolist()) == list(I.D_STOPS), (bf, amp_end, v)
            sel = (ls.bf == bf) & (ls.a_end == amp_end)
            if far:
                assert set(I.D_FAR) <= set(stops[sel].tolist()), (bf, amp_end)
                assert set(k + len(I.D_TRAIN) for k in I.D_FAR) <= set(stops[sel].tolist()), (bf, amp_end)
    # where the dimmed symbol lies relative to a block edge j >= 2 (the sink decides it in a later block than the lock)
    where = {}
    for c in range(ls.n):
        bf = int(ls.bf[c])
        p = int(geo.ci[c]) + int(stops[c]) * bf                 # the dimmed symbol is [p, p + bf)
        for j in range(max(2, p // B), (p + 2 * bf) // B + 1):
            e = j * B
            kind = ("straddles" if p < e < p + bf else "last_before" if p + bf <= e < p + 2 * bf else
                    "first_after" if p - bf < e <= p else None)
            if kind:
                where.setdefault((bf, int(variant[c])), set()).add(kind)
    every = {"first_after", "straddles", "last_before"}
    union = lambda bf: set().union(*(where.get((bf, v), set()) for v in range(3)))  # noqa: E731
    if far:
        # (bit_frames 8: the far stop that is the last symbol before sample 32768 has lead 0, so the next one ends on
        # the edge, not behind it; the rows added around symbol 512 have all three)
        assert union(40) == every and {"first_after", "straddles"} <= union(8), where
    else:
        for bf in (40, 100):
            for v in range(3):
                assert where.get((bf, v), set()) == every, (bf, v, where.get((bf, v)))
        assert union(8) == every, where                        # (the rows added around symbol 512)
    return geo


# --------------------------------------------------------------------------------------------------------- (D)
D_RATES = I.E_RATES                 # 40, 100
D_WORDS = [w for i in range(128) for w in (i, (i + 64) % 128)]     # every 7-bit word in an even and in an odd slot
_VALID = {tuple(G.coded(bytes([n]))[7:]) for n in range(16)}       # the sixteen codewords


def _word_bits(w):
    return [(w >> (6 - b)) & 1 for b in range(7)]


@functools.lru_cache(maxsize=None)
def set_d():
    """``sweep_e``'s streams, and per rate one whose 256 codeword slots hold every 7-bit word as a high and as a low
    nibble: no error, every single error, and every double and triple error."""
    sw = I.sweep_e()
    rows = [(sw.flat[int(sw.off[s]): int(sw.off[s]) + int(sw.ln[s])], int(sw.bf[s]), 14000, dict(every_word=0))
            for s in range(len(sw.meta))]
    bits = [b for w in D_WORDS for b in _word_bits(w)]
    for i, bf in enumerate(D_RATES):
        rows.append((G.stream(G.training(20, bool(i)), bits, bf, lead=4 + i), bf, 14000, dict(every_word=1)))
    return assemble(rows)


def decided_bits(ls, want, c):
    """The data bits the oracle decided in row c's burst."""
    w = want[c][0]
    s, _, _ = O.decode_bits(ls.host[c, w["start"]: w["start"] + w["len"]], 48000 // int(ls.bf[c]), int(ls.a_end[c]))
    assert len(s) == w["nbits"]
    return [int(ch) for ch in s]


def check_d(ls, want):
    geo = geometry(ls, want)
    assert all(w[0]["status"] == ST_OK for w in want) and set((geo.first & 1).tolist()) == {0, 1}
    every = ls.col("every_word") == 1
    assert (geo.nbits[every] == 7 * 256).all() and (geo.nbits[~every] == 14 * I.E_PAYLOAD).all()
    for bf in D_RATES:
        pending, straddled = set(), 0
        for c in np.nonzero(ls.bf == bf)[0]:
            first, nbits, ci = int(geo.first[c]), int(geo.nbits[c]), int(geo.ci[c])
            taken = [committed(geo, ls.bf, c, j) - first for j in range(2, int(geo.ln[c]) // B + 1)]
            taken = [t for t in taken if 0 < t < nbits]         # edges inside the data
            pending |= {t % 14 for t in taken}
            bits = decided_bits(ls, want, c)
            words = [tuple(bits[7 * s: 7 * s + 7]) for s in range(nbits // 7)]
            if every[c]:
                even, odd = words[0::2], words[1::2]
                assert len(set(even)) == 128 and len(set(odd)) == 128
                assert want[c][0]["corrected"] == 256 - 2 * len(_VALID)
            # codewords with a non-zero syndrome that an edge cuts: some of their bits pending across the edge
            straddled += sum(1 for t in taken if t % 7 and words[t // 7] not in _VALID)
        assert pending == set(range(14)), (bf, pending)
        assert straddled >= 2, bf
    return geo


# --------------------------------------------------------------------------------------------------------- (E)
E_RATES = (8, 40, 100, 160, 300, 600, 2000)     # the smallest, and one per lanes-per-symbol value 1, 2, 4, 8, 16, 32
E_CLASSES = ("lt_same_quotient", "lt_other_quotient", "tie", "gt_within_bf", "gt_beyond_bf")
# bit_frames 8 with at most two dead-zone samples (dead_cap): |l2 - l1| = 1 takes both as m1 or m2, nothing is left to
# steer
# M % 8, and M = 65535 n + 65534 with n = 1 ... 5 has M % 8 in 1 ... 5 -- never the >= 6 that S = M + 2 needs to reach
# the next quotient
E_MISSING = {8: ("lt_other_quotient",)}
E_MIN = 8
E_SYMBOLS = {8: 1200, 40: 400, 100: 400, 160: 400, 300: 300, 600: 150, 2000: 48}
E_LEADS = {8: (0, 3), 40: (0, 5), 100: (0, 7), 160: (0, 9), 300: (0, 11), 600: (0, 13), 2000: (0, 15)}
E_EDGE_VALUES = (512, 513, -512, -513)


def symbol_sums(x, bf):
    """(M, S): the sums of |tone - limited| over a symbol's bf samples for the mark and the space tone (ref:342-351),
    in plain numpy."""
    x = np.asarray(x, np.int64)
    lim = np.where(x > 512, 32767, np.where(x < -512, -32768, 0))
    tone = G.tones(bf).astype(np.int64)
    return int(np.abs(tone[1] - lim).sum()), int(np.abs(tone[0] - lim).sum())


def symbol_class(M, S, bf):
    if M < S:
        return "lt_same_quotient" if M // bf == S // bf else "lt_other_quotient"
    if M == S:
        return "tie"
    return "gt_within_bf" if M - S < bf else "gt_beyond_bf"


def dead_cap(bf):
    """Dead-zone samples allowed in one quarter of a symbol: a quarter of the quarter, so that every symbol stays far
    above both squelch thresholds and every block above the gate.  bit_frames 8 (two samples per quarter) could then
    have none: there the whole symbol may hold two, which |l2 - l1| = 1 needs in one quarter."""
    return 2 if bf == 8 else bf // 16


def _craft(rng, bf, want):
    """One symbol of three kinds of samples -- high (> 512), low (< -512) and dead zone -- of the class ``want``, or
    None when this draw cannot reach it.  Per quarter i the counts are (h, l, m).  With m2 - m1 = -2 (l2 - l1) the
    65535s cancel and M - S = 2 (l2 - l1); quarters 0 and 3 add the same to M and S and steer M % bf."""
    q = bf // 4
    cap = dead_cap(bf)
    budget = 2 if bf == 8 else 4 * cap                          # dead-zone samples in the whole symbol
    if want == "gt_beyond_bf":
        # a space symbol with dead-zone samples sprinkled in
        cnt = [[q, 0, 0], [q, 0, 0], [0, q, 0], [0, q, 0]]
        for _ in range(int(rng.integers(0, budget + 1))):
            i = int(rng.integers(0, 4))
            if cnt[i][2] < cap:
                cnt[i][0 if i < 2 else 1] -= 1
                cnt[i][2] += 1
    else:
        dmax = max(1, min(cap // 2, 6))
        d = {"tie": 0, "gt_within_bf": int(rng.integers(1, dmax + 1))}.get(want, -int(rng.integers(1, dmax + 1)))
        assert 2 * abs(d) <= min(cap, budget) and 2 * abs(d) < bf
        spare = budget - 2 * abs(d)
        mm = int(rng.integers(0, min(spare // 2, cap - 2 * abs(d)) + 1))     # dead-zone samples quarters 1, 2 share
        m1, m2 = (mm + 2 * d, mm) if d > 0 else (mm, mm - 2 * d)
        spare -= 2 * mm
        lo = max(0, -d)
        hi = min(q - m1, q - m2 - d)
        if hi < lo:
            return None
        l1 = int(rng.integers(lo, hi + 1))
        l2 = l1 + d
        quarter12 = [[q - l1 - m1, l1, m1], [q - l2 - m2, l2, m2]]
        # steer M % bf: every (l0, m0, m3) within the cap and the budget, l3 drawn once
        g = min(spare, cap, 6)
        l0, m0, m3 = np.meshgrid(np.arange(q + 1), np.arange(g + 1), np.arange(g + 1), indexing="ij")
        ok = (m0 + m3 <= spare) & (l0 + m0 <= q)
        l3 = int(rng.integers(0, q + 1))
        ok &= l3 + m3 <= q
        M = (65535 * l0 + 32767 * m0 + 65535 * (quarter12[0][0]) + 32768 * m1 + 65535 * l2 + 32767 * m2
             + 65535 * (q - l3 - m3) + 32768 * m3)
        S = M - 2 * d
        if want == "lt_same_quotient":
            ok &= M // bf == S // bf
        elif want == "lt_other_quotient":
            ok &= M // bf != S // bf
        pick = np.argwhere(ok)
        if not len(pick):
            return None
        a, b, c = pick[int(rng.integers(0, len(pick)))]
        a, b, c = int(l0[a, b, c]), int(m0[a, b, c]), int(m3[a, b, c])
        cnt = [[q - a - b, a, b], quarter12[0], quarter12[1], [q - l3 - c, l3, c]]
    x = np.empty(bf, np.int64)
    for i, (h, l, m) in enumerate(cnt):
        assert h >= 0 and l >= 0 and 0 <= m <= cap and h + l + m == q
        v = np.concatenate([rng.integers(26000, 32768, h), -rng.integers(26000, 32769, l), rng.integers(-512, 513, m)])
        x[i * q:(i + 1) * q] = rng.permutation(v)
    # the limiter's exact edges: 513 is high, -513 low, 512 and -512 dead zone (two samples of a symbol at the most,
    # one at bit_frames 8: the symbol stays above 14000)
    for _ in range(1 if bf == 8 else 2):
        p = int(rng.integers(0, bf))
        x[p] = 513 if x[p] > 512 else (-513 if x[p] < -512 else int(rng.choice([512, -512])))
    assert int(np.abs(x).sum()) >= 14000 * bf and (np.abs(x) <= 512).sum() <= budget
    return x


@functools.lru_cache(maxsize=None)
def set_e():
    rng = np.random.default_rng(5005)
    rows = []
    for bf in E_RATES:
        train = G.training(1 if bf == 2000 else 20)
        classes = [k for k in E_CLASSES if k not in E_MISSING.get(bf, ())]
        for lead in E_LEADS[bf]:
            syms, tries = [], 0
            while len(syms) < E_SYMBOLS[bf]:
                x = _craft(rng, bf, classes[len(syms) % len(classes)])
                tries += 1
                assert tries < 50 * E_SYMBOLS[bf], (bf, classes[len(syms) % len(classes)])
                if x is not None:
                    syms.append(x)
            order = rng.permutation(len(syms))
            body = np.concatenate([syms[i] for i in order]).astype(np.int16)
            x = np.concatenate([G.render(train, bf, lead=lead), body, np.zeros(12 * bf, np.int16)])
            rows.append((x, bf, 14000, dict(lead=lead, crafted=len(syms))))
    return assemble(rows)


def check_e(ls, want):
    """Also returns the classes found per rate."""
    geo = geometry(ls, want)
    assert geo.ci.tolist() == ls.col("lead").tolist()
    # every crafted symbol above the squelch, every block above the gate: one burst (geometry), nbits = all of them
    assert geo.nbits.tolist() == ls.col("crafted").tolist() and all(w[0]["status"] == ST_OK for w in want)
    found = {}
    seen = set()
    for c in range(ls.n):
        bf, w = int(ls.bf[c]), want[c][0]
        burst = ls.host[c, w["start"]: w["start"] + w["len"]]
        nsym = int(geo.first[c] + geo.nbits[c])
        r = O.demod_batch_soft(burst, [0], [len(burst)], [bf], int(ls.a_end[c]), out_stride=8, margin_stride=nsym)
        assert int(r["n_symbols"][0]) == nsym
        bits = decided_bits(ls, want, c)
        count = found.setdefault(bf, dict.fromkeys(E_CLASSES, 0))
        for i in range(int(geo.nbits[c])):
            k = int(geo.first[c]) + i
            x = burst[int(geo.ci[c]) + k * bf: int(geo.ci[c]) + (k + 1) * bf]
            M, S = symbol_sums(x, bf)
            assert int(r["margins"][0, k]) == S // bf - M // bf, (c, k)
            assert bits[i] == int(M // bf < S // bf), (c, k)
            dead = (np.abs(x.reshape(4, -1).astype(np.int64)) <= 512).sum(axis=1)
            assert dead.max() <= dead_cap(bf) and dead.sum() <= bf // 4, (c, k, dead)
            count[symbol_class(M, S, bf)] += 1
            seen |= set(x.tolist()) & set(E_EDGE_VALUES)
    for bf in E_RATES:
        for k in E_CLASSES:
            if k in E_MISSING.get(bf, ()):
                assert found[bf][k] == 0, (bf, k)
            else:
                assert found[bf][k] >= E_MIN, (bf, k, found[bf])
    assert seen == set(E_EDGE_VALUES)
    return found


# ------------------------------------------------------------------------------------- flat batches and the thin mix

def as_sweep(ls, want, rows):
    """The bursts of ``rows`` as a flat batch (``split_sweep_inputs.Sweep``) for the batch and split entries."""
    return I.assemble([(np.ascontiguousarray(ls.host[c, want[c][0]["start"]: want[c][0]["start"] + want[c][0]["len"]]),
                        int(ls.bf[c]), dict(row=int(c))) for c in rows])


@functools.lru_cache(maxsize=None)
def mix(far):
    """A thinned mix of (B), (C) and (D) at interleaved rates: every seventh row, and every row whose placement is an
    edge case -- the terminator ending on an edge or split by the edge between blocks 1 and 2, a false terminator, a
    dimmed symbol within a symbol of an edge behind the lock, the every-word streams.  ``far``: the far stops of (C)
    instead, which are many times as long, with all of (D)'s rows between them (without ``far``: its shorter ones)."""
    keep = []
    for name in ("c_far", "d") if far else ("b", "c", "d"):
        ls, want = load(name)
        geo = geometry(ls, want)
        edge = np.zeros(ls.n, bool)
        for r in range(ls.n):
            bf = int(ls.bf[r])
            m = ls.meta[r]
            if m.get("on_edge") or m.get("false") or m.get("every_word") or m.get("extra") or m.get("far"):
                edge[r] = True
            elif name == "b":
                done = committed(geo, ls.bf, r, 2) - (int(geo.first[r]) - 4)
                edge[r] = 0 < done < 4
            elif name == "c":
                p = int(geo.ci[r]) + int(geo.first[r] + geo.nbits[r] - (I.D_LATER if m["variant"] == 2 else 0)) * bf
                edge[r] = p >= 2 * B - bf and min(p % B, -p % B) < bf and m["variant"] > 0
        rows = np.nonzero(edge | (np.arange(ls.n) % 7 == 0))[0]
        if name == "d" and not far:
            rows = np.nonzero(geo.ln <= 40 * B)[0]              # (the rows at bit_frames 100 go with the far ones)
        keep.append(subset(ls, rows))
    ls = concat(keep)
    order = np.random.default_rng(5006).permutation(ls.n)      # the rates interleaved
    return subset(ls, order)


SETS = {"a": set_a, "b": set_b, "c": lambda: set_c(False), "c_far": lambda: set_c(True), "d": set_d, "e": set_e,
        "mix": lambda: mix(False), "mix_far": lambda: mix(True)}


@functools.lru_cache(maxsize=None)
def load(name):
    """(the set, its expected rows), computed once per process."""
    ls = SETS[name]()
    return ls, expected(ls)
