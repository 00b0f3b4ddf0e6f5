"""A pure-Python model of the streaming live receiver's demodulator (afsk_live_stream.hip): one burst fed one
2048-sample block at a time, keeping only what the next block needs -- the first block until the clock index is known,
then the samples of the symbols not yet committed.  tests/test_live_stream_host.py pins it against the CPU oracle's
demod_batch; it states the incremental rules the device code follows (the K rule, the terminator window, whole
codewords, whole bytes).  Not a test module."""
from __future__ import annotations

import numpy as np

from afskmodem_amd import _native
from oracle import afsk_oracle as O

BLOCK = 2048
SYNC = 4096
H = ((1, 0, 1, 0, 1, 0, 1), (0, 1, 1, 0, 0, 1, 1), (0, 0, 0, 1, 1, 1, 1))


def symbols(x, bf, amp_end):
    """(decisions, loud flags) of the rows of x ([n, bf] samples, one symbol each): the quarter sums of
    split_segment_rt_kernel."""
    x = np.asarray(x, np.int64).reshape(-1, bf)
    q = bf // 4
    h = np.where(x > 512, 0, np.where(x < -512, 65535, 32767)).reshape(-1, 4, q).sum(axis=2)
    full = 65535 * q
    md = (2 * full + h[:, 0] + h[:, 2] - h[:, 1] - h[:, 3]) // bf
    sd = (2 * full + h[:, 0] + h[:, 1] - h[:, 2] - h[:, 3]) // bf
    thr = min(max(amp_end, 0), 40000) * bf
    return (md < sd).astype(int).tolist(), (np.abs(x).sum(axis=1) >= thr).tolist()


def symbol(x, bf, amp_end):
    """(decision, loud) of one symbol's bf samples."""
    d, loud = symbols(x, bf, amp_end)
    return d[0], loud[0]


def hamming(cw_bits):
    r = list(cw_bits)
    s = [sum(a * b for a, b in zip(row, r)) % 2 for row in H]
    pos = s[2] * 4 + s[1] * 2 + s[0]
    if pos:
        r[pos - 1] ^= 1
    return pos != 0, (r[2] << 3) | (r[4] << 2) | (r[5] << 1) | r[6]


class StreamDemodModel:
    """One burst of one channel at bit_frames ``bf``."""

    def __init__(self, bf: int, amp_end: int = 14000, max_payload_len: int = 256):
        self.bf, self.amp_end, self.max_payload = bf, amp_end, max_payload_len
        self.phase = 0              # 0 = fewer than 4096 samples, 1 = terminator search, 2 = data, 3 = stopped
        self.length = 0             # samples fed
        self.keep = np.zeros(0, np.int16)
        self.keep_from = 0          # burst position of keep[0]
        self.ci = -1
        self.k = 0
        self.first = 0
        self.hist = [0, 0, 0]
        self.pend = []
        self.nbits = 0
        self.ncw = 0
        self.corrected = 0
        self.hi = 0
        self.payload = bytearray()

    def feed(self, block) -> None:
        block = np.asarray(block, np.int16)
        assert block.size == BLOCK
        self.keep = np.concatenate([self.keep, block])
        self.length += BLOCK
        if self.length > _native.MAX_STREAM_LEN or self.phase == 3:
            self.keep = self.keep[:0]
            return
        if self.length < SYNC:
            return
        if self.phase == 0:
            assert self.keep_from == 0 and self.keep.size == SYNC
            self.ci = O.recover_clock_index(self.keep, 48000 // self.bf)
            self.phase, self.k = 1, 0
        bf = self.bf
        k_end = (self.length - self.ci - 1) // bf          # symbols with ci + (k + 1) * bf < len
        p = self.ci + self.k * bf - self.keep_from
        assert p >= 0 or self.k >= k_end, "a symbol's samples were dropped"
        dec, loud = symbols(self.keep[p:p + max(k_end - self.k, 0) * bf], bf, self.amp_end)
        for d, l in zip(dec, loud):                         # (the block's complete symbols, decided at once)
            if self.phase == 3:
                break
            self._commit(d, l)
            self.k += 1
        # what the next block needs: the uncommitted symbol's samples (at most bf)
        start = self.ci + self.k * bf
        self.keep = self.keep[start - self.keep_from:]
        self.keep_from = start
        assert self.keep.size <= bf or self.phase == 3

    def _commit(self, d: int, loud: bool) -> None:
        if self.phase == 1:
            if self.hist + [d] == [1, 0, 0, 0]:
                self.first, self.phase = self.k + 1, 2
            self.hist = (self.hist + [d])[1:]
            return
        if not loud:
            self.phase = 3
            return
        self.nbits += 1
        self.pend.append(d)
        if len(self.pend) == 7:
            bad, nib = hamming(self.pend)
            self.pend = []
            self.corrected += bad
            if self.ncw & 1:
                if (self.ncw >> 1) < self.max_payload:
                    self.payload.append((self.hi << 4) | nib)
            else:
                self.hi = nib
            self.ncw += 1

    def result(self) -> dict:
        """The burst's DemodOutputs as the streaming receiver reports them."""
        if self.length > _native.MAX_STREAM_LEN:
            return dict(nbytes=0, nbits=0, clock_idx=-1, term_frame=-1, status=_native.ST_BAD_LENGTH, corrected=0,
                        bytes=b"")
        if self.phase == 0:
            return dict(nbytes=0, nbits=0, clock_idx=-1, term_frame=-1, status=_native.ST_TOO_SHORT, corrected=0,
                        bytes=b"")
        nbits = 0 if self.phase == 1 else self.nbits
        term = self.ci + (self.k if self.phase == 1 else self.first) * self.bf
        return dict(nbytes=(nbits // 7) >> 1, nbits=nbits, clock_idx=self.ci, term_frame=term,
                    status=_native.ST_NO_DATA if nbits == 0 else _native.ST_OK,
                    corrected=0 if self.phase == 1 else self.corrected, bytes=bytes(self.payload))


def demod_streaming(burst, bf: int, amp_end: int = 14000, max_payload_len: int = 256) -> dict:
    """Feed a burst (a multiple of 2048 samples) block by block and return the model's result."""
    burst = np.asarray(burst, np.int16)
    assert burst.size % BLOCK == 0
    m = StreamDemodModel(bf, amp_end, max_payload_len)
    for b in range(burst.size // BLOCK):
        m.feed(burst[b * BLOCK:(b + 1) * BLOCK])
    return m.result()
