"""Symbol-level stream generator for the boundary sweeps (tests/split_sweep_inputs.py).  Not a test module.

A stream is written as the list of symbols a receiver will decide on, one oracle tone per symbol, so that a test can
put the terminator, a quiet symbol or a flipped coded bit at an exact symbol index.  Pure numpy plus the oracle's
tones.  What a stream decodes to is never taken from here: the sweeps ask the oracle, and check from the oracle's
outputs that every placement they were built for happened (clock index = the lead-in, terminator where intended).
tests/live_sweep_inputs.py builds the streaming live receiver's sweeps (gate-block edges, near-tie symbols) on it,
too."""
import functools

import numpy as np

from oracle import afsk_oracle as O

SYNC_WINDOW = 4096                 # a shorter stream is refused (ref:323-325)

# Hamming(7,4), codeword = p1 p2 d1 p3 d2 d3 d4 (ref:115-123)
_GENERATOR = np.array([[1, 1, 0, 1], [1, 0, 1, 1], [1, 0, 0, 0], [0, 1, 1, 1],
                       [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.uint8)


@functools.lru_cache(maxsize=None)
def tones(bf):
    """int32 [2, bf]: row 0 the space tone, row 1 the mark tone of the rate with ``bf`` samples per symbol."""
    baud = 48000 // bf
    assert baud * bf == 48000
    space, mark = O.space_tone(baud), O.mark_tone(baud)
    assert space.size == bf and mark.size == bf and space[0] > 0 and mark[0] > 0
    return np.stack([space, mark]).astype(np.int32)


def render(bits, bf, level=None, lead=0):
    """int16 samples: ``lead`` zeros, then one symbol per entry of ``bits`` (mark for 1, space for 0).
    ``level[k] = (a, d)``: symbol k keeps its signs at magnitude a, its first sample is a + d, so the symbol's
    sum of |x| is a * bf + d -- exactly on (d = 0), one below or one above a squelch threshold a.  (0, 0): silent."""
    b = np.asarray(bits, np.int64).reshape(-1)
    assert b.size == 0 or (b.min() >= 0 and b.max() <= 1)
    sym = tones(bf)[b]                                     # [n, bf], a copy
    for k, (a, d) in (level or {}).items():
        assert 0 <= k < b.size and 0 <= a and 0 <= a + d and a <= 32767 and a + d <= 32767
        s = np.sign(sym[k]) * int(a)
        s[0] = int(a) + int(d)                             # (both tones start on their positive half)
        sym[k] = s
        assert int(np.abs(s).sum()) == int(a) * bf + int(d)
    out = np.concatenate([np.zeros(int(lead), np.int32), sym.reshape(-1)])
    return np.clip(out, -32768, 32767).astype(np.int16)


def training(c, even=False):
    """c training cycles and the terminator 1,0,0,0.  ``even``: 1,1,0,0,0 instead -- the scan takes the first 1,0,0,0
    anywhere, so the terminator's last symbol then has an even index (a transmitter's is always odd)."""
    return [1, 0] * int(c) + ([1, 1, 0, 0, 0] if even else [1, 0, 0, 0])


def training_ending_at(kt):
    """The training whose terminator's last symbol has index kt (>= 3)."""
    return training((kt - 4) // 2, True) if kt % 2 == 0 else training((kt - 3) // 2, False)


def coded(payload):
    """The 14 coded bits per payload byte (two Hamming codewords, high nibble first), as a list of 0 / 1."""
    data = np.frombuffer(bytes(payload), np.uint8)
    nib = np.unpackbits(data).reshape(-1, 4)
    return ((nib @ _GENERATOR.T) & 1).astype(np.uint8).reshape(-1).tolist()


def flip(bits, positions):
    """A copy of ``bits`` with the entries at ``positions`` inverted (single-bit Hamming errors where wanted)."""
    out = list(bits)
    for p in positions:
        out[p] ^= 1
    return out


def stream(train, data, bf, lead=0, level=None, tail=12, min_len=SYNC_WINDOW):
    """``render`` of training + data with ``tail`` silent symbols behind, padded with silence to ``min_len`` samples.
    The keys of ``level`` count from the first DATA symbol."""
    first = len(train)
    lv = {first + k: v for k, v in (level or {}).items()}
    x = render(list(train) + list(data), bf, lv, lead)
    pad = max(tail * bf, min_len - len(x))
    return np.concatenate([x, np.zeros(pad, np.int16)])
