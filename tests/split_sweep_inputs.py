"""Input sets of the split-path boundary sweeps (tests/test_gpu_split_sweeps.py) and the placement conditions each
set was built for.  Not a test module.

Every set is a ``Sweep``: a flat sample buffer, per-stream offset / length / bit_frames, and per stream what the
generator (tests/symbol_streams.py) INTENDED.  The expected outputs are the oracle's (``reference``); the
``check_*`` functions assert, from the oracle's outputs alone, that the placement happened -- all eight alignment
forms for both offset parities, every residue of the symbol count, every terminator index, every stop position -- so
a drifting generator fails loudly instead of quietly covering less.  tests/test_symbol_streams_host.py runs these
checks on the CPU; the GPU sweeps run them again on the very results they compare against.

Streams that are one signal cut at several lengths share their samples (same offset, different length): the
demodulators only read."""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import afsk_oracle as O
from tests import symbol_streams as G

RATES = (40, 8, 100)               # LDS-DMA kernel; run-time kernel with q = 2 and with q = 25 (odd)
ST_OK, ST_TOO_SHORT, ST_NO_DATA = 0, 1, 2


@dataclass
class Sweep:
    flat: np.ndarray               # int16
    off: np.ndarray                # int64 [n]
    ln: np.ndarray                 # int32 [n]
    bf: np.ndarray                 # int32 [n]
    meta: list                     # [n] dicts: what the generator intended

    def col(self, key, default=-1):
        return np.array([m.get(key, default) for m in self.meta], np.int64)

    @property
    def stride(self):
        """Bytes per output row that hold every stream's whole payload."""
        return int(np.max(self.ln // (14 * self.bf))) + 8


def _pack(xs):
    from tests.test_gpu_split import _pack as pack
    return pack(xs, odd_gap=True)


def assemble(bases):
    """bases: (samples, bit_frames, cuts) with cuts = [(length, meta), ...] -- or None for the whole signal with
    the meta given in its place.  Signals are laid out back to back with a spare sample in front of every other one
    (odd offsets); the cuts of one signal share its offset."""
    flat, boff, _ = _pack([b[0] for b in bases])
    off, ln, bf, meta = [], [], [], []
    for (x, f, cuts), o in zip(bases, boff):
        if isinstance(cuts, dict):
            cuts = [(len(x), cuts)]
        for L, m in cuts:
            assert 0 <= L <= len(x)
            off.append(int(o)); ln.append(int(L)); bf.append(f); meta.append(m)
    return Sweep(flat, np.array(off, np.int64), np.array(ln, np.int32), np.array(bf, np.int32), meta)


def subset(sw, idx):
    idx = np.asarray(idx)
    return Sweep(sw.flat, sw.off[idx], sw.ln[idx], sw.bf[idx], [sw.meta[i] for i in idx])


def concat(a, b):
    return Sweep(np.concatenate([a.flat, b.flat]), np.concatenate([a.off, b.off + a.flat.size]),
                 np.concatenate([a.ln, b.ln]), np.concatenate([a.bf, b.bf]), a.meta + b.meta)


def oracle(sw, amp_end=14000, ln=None, soft=None):
    """The oracle's outputs for ``sw`` (at the lengths ``ln`` when given); ``soft`` = margin_stride: also corrected,
    margins and n_symbols."""
    ln = sw.ln if ln is None else ln
    if soft is not None:
        return O.demod_batch_soft(sw.flat, sw.off, ln, sw.bf, amp_end, out_stride=sw.stride, margin_stride=soft)
    return O.demod_batch(sw.flat, sw.off, ln, sw.bf, amp_end, out_stride=sw.stride, n_threads=8)


def geometry(sw, want, ln=None):
    """(ci, first, K) per stream from the oracle's outputs: the clock index, the first data symbol and the number of
    symbols with i < len - bf (ref:362, 372)."""
    ln = (sw.ln if ln is None else ln).astype(np.int64)
    ci, tf, bf = want["clock_idx"].astype(np.int64), want["term_frame"].astype(np.int64), sw.bf.astype(np.int64)
    return ci, (tf - ci) // bf, (ln - ci - 1) // bf


def _payload(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


# --------------------------------------------------------------------------------------------------------- (a)
A_SEGMENTS = (64, 128, 192, 256, 320, 1024)     # 1, 2, 3, 4, 5 and >= 5 passes in the first segment
A_PAYLOAD = 40                                  # 64 training symbols + 560 coded bits: K >= 6 * 64 + 40


@functools.lru_cache(maxsize=None)
def sweep_a():
    """bit_frames 40: lead-ins 0 ... 15 (ci & 7 twice over), ordered so that the low eight land on even and the high
    eight on odd stream offsets."""
    rng = np.random.default_rng(4001)
    pools = {0: list(range(8)), 1: list(range(8, 16))}
    bases, pos = [], 0
    for i in range(16):
        pos += i % 2                                            # the spare sample of _pack(odd_gap=True)
        pool = pools[pos & 1] or pools[1 - (pos & 1)]
        lead = pool.pop(0)
        x = G.stream(G.training(30), G.coded(_payload(rng, A_PAYLOAD)), 40, lead=lead)
        if len(x) % 2:
            x = np.concatenate([x, np.zeros(1, np.int16)])
        bases.append((x, 40, dict(lead=lead, nbits=14 * A_PAYLOAD)))
        pos += len(x)
    return assemble(bases)


def check_a(sw, want):
    ci, first, K = geometry(sw, want)
    for parity in (0, 1):
        sel = (sw.off & 1) == parity
        assert set((ci[sel] & 7).tolist()) == set(range(8)), (parity, ci[sel])
    assert ci.tolist() == sw.col("lead").tolist()
    assert (K >= 6 * 64 + 40).all()
    assert want["nbits"].tolist() == sw.col("nbits").tolist() and (want["status"] == ST_OK).all()
    assert (want["nbytes"] == A_PAYLOAD).all()


# --------------------------------------------------------------------------------------------------------- (b)
B_RATES = (40, 8, 100, 2000)
B_LEADS = (0, 5)


@functools.lru_cache(maxsize=None)
def sweep_b(straddle):
    """One loud signal per rate and lead-in, cut so that K takes 64 consecutive values -- just past the terminator,
    or (``straddle``) around symbol 1024, the default segment's edge -- and cut at the lengths around one K."""
    rng = np.random.default_rng(4002 + int(straddle))
    bases = []
    for bf in B_RATES:
        train = G.training(1 if bf == 2000 else 30)
        first = len(train)
        K0 = 992 if straddle else max(first + 6, G.SYNC_WINDOW // bf + 8)
        Km = 1024 if straddle else K0 + 17
        for lead in B_LEADS:
            data = rng.integers(0, 2, K0 + 66 - first).tolist()
            x = G.render(train + data, bf, lead=lead)
            cuts = [(lead + K * bf + 1, dict(K=K, lead=lead, first=first)) for K in range(K0, K0 + 64)]
            # the last-symbol rule i < len - bf: K symbols from len = ci + K bf + 1 to ci + K bf + bf
            cuts += [(lead + Km * bf + e, dict(K=Km, lead=lead, first=first)) for e in (1, bf - 1, bf)]
            cuts += [(lead + Km * bf, dict(K=Km - 1, lead=lead, first=first))]
            assert all(L >= G.SYNC_WINDOW for L, _ in cuts)
            bases.append((x, bf, cuts))
    return assemble(bases)


def check_b(sw, want, straddle):
    ci, first, K = geometry(sw, want)
    assert ci.tolist() == sw.col("lead").tolist() and first.tolist() == sw.col("first").tolist()
    assert K.tolist() == sw.col("K").tolist()
    for bf in B_RATES:
        for lead in B_LEADS:
            sel = (sw.bf == bf) & (ci == lead)
            assert set((K[sel] & 63).tolist()) == set(range(64)), (bf, lead)
            if straddle:
                assert {1023, 1024, 1025} <= set(K[sel].tolist()), (bf, lead)
    assert (want["nbits"] == K - first).all() and (want["status"] == ST_OK).all()      # no squelch stop


# --------------------------------------------------------------------------------------------------------- (c)
C_SEGMENTS = (64, 128, 1024)
C_NEAR = tuple(range(60, 201))                  # words 0 ... 3, every straddle of a word edge
C_FAR = tuple(range(4090, 4103))                # stage C searches 64 words at a time: symbol 4096
C_FALSE = (64, 66, 127)                         # k & 63 = 0, 2, 63
C_PAYLOAD = 20


@functools.lru_cache(maxsize=None)
def sweep_c():
    rng = np.random.default_rng(4003)
    bases = []
    for bf in RATES:
        kts = C_NEAR + (C_FAR if bf in (40, 8) else ())
        for i, kt in enumerate(kts):
            x = G.stream(G.training_ending_at(kt), G.coded(_payload(rng, C_PAYLOAD)), bf, lead=i % 6)
            bases.append((x, bf, dict(kt=kt, nbits=14 * C_PAYLOAD, lead=i % 6)))
        for i, kt in enumerate(C_FALSE):
            # a data-like 1,0,0,0 inside the training: the scan stops there, the rest of the training is data
            rest = [1, 0] * 20 + [1, 0, 0, 0]
            x = G.stream(G.training_ending_at(kt) + rest, G.coded(_payload(rng, C_PAYLOAD)), bf, lead=i)
            bases.append((x, bf, dict(kt=kt, nbits=len(rest) + 14 * C_PAYLOAD, lead=i, false=1)))
    return assemble(bases)


def check_c(sw, want):
    ci, first, K = geometry(sw, want)
    kt = first - 1
    assert ci.tolist() == sw.col("lead").tolist()
    assert kt.tolist() == sw.col("kt").tolist()
    for bf in RATES:
        sel = sw.bf == bf
        true = sel & (sw.col("false", 0) == 0)
        assert set(kt[true].tolist()) == set(C_NEAR + (C_FAR if bf in (40, 8) else ())), bf
        assert sorted(kt[sel & ~true].tolist()) == sorted(C_FALSE), bf
        assert {0, 1, 2, 3} <= set((kt[true] & 63).tolist())
    assert want["nbits"].tolist() == sw.col("nbits").tolist() and (want["status"] == ST_OK).all()


# --------------------------------------------------------------------------------------------------------- (d)
D_AMP_ENDS = (14000, 9000)
D_SEGMENTS = (64, 1024)
D_TRAIN = G.training(20)                        # first data symbol 44: the stop search's first word is masked
D_STOPS = tuple(range(141))                     # data symbols 0 ... 140: absolute 44 ... 184, words 0, 1 and 2
D_LATER = 70                                    # the on-threshold variant is ended by a silent symbol this much later
D_FAR = tuple(range(4090, 4103))


def _dimmed(j, variant, amp_end):
    """(level, intended nbits) for a first dimmed data symbol j: silent; one below the threshold (stops); on the
    threshold (does not stop: a silent symbol D_LATER on does)."""
    if variant == 0:
        return {j: (0, 0)}, j
    if variant == 1:
        return {j: (amp_end, -1)}, j
    return {j: (amp_end, 0), j + D_LATER: (0, 0)}, j + D_LATER


@functools.lru_cache(maxsize=None)
def sweep_d(amp_end):
    rng = np.random.default_rng(4004)
    first = len(D_TRAIN)
    bases = []
    for bf in RATES:
        data = G.coded(_payload(rng, 24))
        for j in D_STOPS:
            for variant in range(3):
                level, nbits = _dimmed(j, variant, amp_end)
                x = G.stream(D_TRAIN, data, bf, lead=j % 4, level=level)
                bases.append((x, bf, dict(nbits=nbits, variant=variant, j=j)))
        # the stop at the very last symbol K - 1 (silent, one below the threshold), and no stop at all: the signal
        # runs past the cut, so the length alone ends the stream
        Kb = -(-max(G.SYNC_WINDOW // bf + 64, first + 64) // 64) * 64
        for Kt in (Kb, Kb + 1, Kb + 63):
            D = Kt - first
            bits = G.coded(_payload(rng, D // 14 + 2))[: D + 1]
            for variant, level in enumerate(({D - 1: (0, 0)}, {D - 1: (amp_end, -1)}, {D - 1: (amp_end, 0)}, None)):
                x = G.stream(D_TRAIN, bits, bf, lead=3, level=level)
                bases.append((x, bf, [(3 + Kt * bf + 1, dict(nbits=D - 1 if variant < 2 else D, K=Kt, end=1))]))
        if bf in (40, 8):
            # the second trip of the stop loop (64 words on from the word of `first`): stops around the ABSOLUTE symbol
            # 4096, where that trip begins, and in [first + 4090, first + 4102]
            data = G.coded(_payload(rng, 600))
            for i, j in enumerate([k - first for k in D_FAR] + list(D_FAR)):
                level, nbits = _dimmed(j, i % 3, amp_end)
                x = G.stream(D_TRAIN, data, bf, lead=i % 4, level=level)
                bases.append((x, bf, dict(nbits=nbits, variant=i % 3, j=j, far=1)))
    return assemble(bases)


def check_d(sw, want):
    ci, first, K = geometry(sw, want)
    assert (first == len(D_TRAIN)).all()
    assert want["nbits"].tolist() == sw.col("nbits").tolist()
    assert (want["status"] == np.where(sw.col("nbits") == 0, ST_NO_DATA, ST_OK)).all()
    j, variant, far = sw.col("j"), sw.col("variant"), sw.col("far", 0)
    for bf in RATES:
        for v in range(3):
            sel = (sw.bf == bf) & (variant == v) & (far == 0) & (j >= 0)
            assert sorted(j[sel].tolist()) == list(D_STOPS), (bf, v)
            # the on-threshold symbol does not stop the decode, the two others do
            assert (want["nbits"][sel] == j[sel] + (D_LATER if v == 2 else 0)).all(), (bf, v)
        end = (sw.bf == bf) & (sw.col("end", 0) == 1)
        assert (K[end] == sw.col("K")[end]).all() and {0, 1, 63} == set((K[end] & 63).tolist())
        assert set((K[end] - first[end] - want["nbits"][end]).tolist()) == {0, 1}        # never, and at K - 1
        if bf in (40, 8):
            stops = (first + j)[(sw.bf == bf) & (far == 1)]
            assert set(D_FAR) <= set(stops.tolist()) and set(k + len(D_TRAIN) for k in D_FAR) <= set(stops.tolist())


# --------------------------------------------------------------------------------------------------------- (e)
E_RATES = (40, 100)
E_SEGMENTS = (64, 1024)
E_PAYLOAD = 96
E_DOUBLE = (2, 100)                             # codewords with TWO flipped bits (2: across a word edge for first = 44)


@functools.lru_cache(maxsize=None)
def sweep_e():
    rng = np.random.default_rng(4005)
    bases = []
    for bf in E_RATES:
        for even in (False, True):
            for double in (False, True):
                bits = G.coded(_payload(rng, E_PAYLOAD))
                single = list(range(0, 2 * E_PAYLOAD, 3))                   # every third codeword: one flipped bit,
                flips = [7 * cw + (n % 7) for n, cw in enumerate(single)]   # its position cycling 0 ... 6
                if double:
                    assert not set(E_DOUBLE) & set(single)
                    flips += [7 * cw + p for cw in E_DOUBLE for p in (1, 4)]
                x = G.stream(G.training(20, even), G.flip(bits, flips), bf, lead=2 + even)
                bases.append((x, bf, dict(double=int(double), flipped=len(single), nbits=14 * E_PAYLOAD,
                                          first=len(G.training(20, even)))))
    return assemble(bases)


def check_e(sw, want):
    """want: the oracle's soft outputs."""
    ci, first, K = geometry(sw, want)
    assert first.tolist() == sw.col("first").tolist() and set((first & 1).tolist()) == {0, 1}
    assert want["nbits"].tolist() == sw.col("nbits").tolist() and (want["nbytes"] == E_PAYLOAD).all()
    single = sw.col("double") == 0
    assert single.any() and (~single).any()
    assert (want["corrected"][single] == sw.col("flipped")[single]).all()
    for s in range(len(sw.meta)):
        sh = (first[s] + 14 * np.arange(E_PAYLOAD)) & 63
        assert (sh > 50).any() and (sh <= 50).any() and set((sh & 1).tolist()) == {int(first[s]) & 1}
        # corrections inside codewords that lie across a word edge
        cw_at = first[s] + 7 * np.arange(0, 2 * E_PAYLOAD, 3)
        assert ((cw_at & 63) > 57).any()
    return K


# --------------------------------------------------------------------------------------------------------- (f)
F_SEGMENT = 64


@functools.lru_cache(maxsize=None)
def sweep_f():
    """A mixed 40 / 8 / 100 batch out of (b) and (d), and the shortened lengths of its fourth launch."""
    b, d = sweep_b(False), sweep_d(14000)
    keep_b = np.nonzero(b.bf != 2000)[0][::3]
    special = np.array([bool(m.get("end") or m.get("far")) for m in d.meta])
    keep_d = np.nonzero(special | (np.arange(len(d.meta)) % 11 == 0))[0]
    sw = concat(subset(b, keep_b), subset(d, keep_d))
    assert set(sw.bf.tolist()) == set(RATES) and (sw.ln >= G.SYNC_WINDOW).all()
    rng = np.random.default_rng(4006)
    short = rng.integers(G.SYNC_WINDOW, sw.ln.astype(np.int64) + 1).astype(np.int32)
    longest = int(np.argmax(sw.ln // sw.bf))
    short[longest] = sw.ln[longest] // 3                    # whole trailing segments are never touched
    short[(longest + 1) % sw.ln.size] = G.SYNC_WINDOW       # the shortest stream that decodes
    refused = [(longest + 2) % sw.ln.size, 0]
    short[refused[0]], short[refused[1]] = G.SYNC_WINDOW - 1, 4000
    return sw, short, longest, refused


def check_f(sw, short, longest, refused, want_short):
    assert (short <= sw.ln).all() and (short < sw.ln).sum() > sw.ln.size // 2
    sym = lambda ln: -(-ln.astype(np.int64) // sw.bf)  # noqa: E731
    assert sym(short)[longest] + 2 * F_SEGMENT < sym(sw.ln)[longest]
    assert (want_short["status"][refused] == ST_TOO_SHORT).all()
    ok = np.ones(sw.ln.size, bool)
    ok[refused] = False
    assert (want_short["status"][ok] != ST_TOO_SHORT).all() and (want_short["nbits"][ok] > 0).sum() > ok.sum() // 2
