"""A pure-Python model of the streaming live receiver's payload tap (afsk_live_tap.hip), built on
tests/live_stream_model.py's StreamDemodModel: the bytes the demodulator commits per fed block (TapDemodModel), and one
channel's gate walk over pushed chunks with the five tap outputs of every push (TapChannelModel).
tests/test_live_tap_host.py pins both against the CPU oracle.  Not a test module."""
from __future__ import annotations

import numpy as np

from afskmodem_amd import _native
from oracle import afsk_oracle as O
from tests.live_stream_model import BLOCK, SYNC, StreamDemodModel, hamming


def tap_cap(max_chunk_len: int, min_bit_frames: int) -> int:
    """AFSK_LIVE_TAP_CAP of include/afsk_amd.h."""
    k = (2047 + max_chunk_len) // 2048
    return ((k + 1) * 2048 // min_bit_frames) // 14 + 1


class TapDemodModel(StreamDemodModel):
    """StreamDemodModel that also keeps every committed byte (``tap``: never truncated by max_payload_len) and
    decides a block's symbols in one numpy pass (the same quarter sums)."""

    def __init__(self, bf: int, amp_end: int = 14000, max_payload_len: int = 256):
        super().__init__(bf, amp_end, max_payload_len)
        self.tap = bytearray()

    def feed(self, block) -> bytes:
        """Feed one block; returns the bytes it committed."""
        before = len(self.tap)
        block = np.asarray(block, np.int16)
        assert block.size == BLOCK
        self.keep = np.concatenate([self.keep, block])
        self.length += BLOCK
        if self.length > _native.MAX_STREAM_LEN or self.phase == 3:
            self.keep = self.keep[:0]
            return b""
        if self.length < SYNC:
            return b""
        if self.phase == 0:
            assert self.keep_from == 0 and self.keep.size == SYNC
            self.ci = O.recover_clock_index(self.keep, 48000 // self.bf)
            self.phase, self.k = 1, 0
        bf = self.bf
        k_end = (self.length - self.ci - 1) // bf          # symbols with ci + (k + 1) * bf < len
        n = k_end - self.k
        if n > 0:
            p = self.ci + self.k * bf - self.keep_from
            assert p >= 0, "a symbol's samples were dropped"
            x = self.keep[p:p + n * bf].astype(np.int64).reshape(n, bf)
            q = bf // 4
            h = np.where(x > 512, 0, np.where(x < -512, 65535, 32767))
            hq = h.reshape(n, 4, q).sum(axis=2)
            full = 65535 * q
            md = (2 * full + hq[:, 0] + hq[:, 2] - hq[:, 1] - hq[:, 3]) // bf
            sd = (2 * full + hq[:, 0] + hq[:, 1] - hq[:, 2] - hq[:, 3]) // bf
            dec = (md < sd).astype(np.int64).tolist()
            loud = (np.abs(x).sum(axis=1) >= min(max(self.amp_end, 0), 40000) * bf).tolist()
            for i in range(n):
                if self.phase == 3:
                    break
                self._commit(dec[i], loud[i])
                self.k += 1
        start = self.ci + self.k * bf
        self.keep = self.keep[start - self.keep_from:]
        self.keep_from = start
        assert self.keep.size <= bf or self.phase == 3
        return bytes(self.tap[before:])

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
                byte = (self.hi << 4) | nib
                self.tap.append(byte)
                if (self.ncw >> 1) < self.max_payload:
                    self.payload.append(byte)
            else:
                self.hi = nib
            self.ncw += 1

    def nbytes(self) -> int:
        return 0 if self.phase < 2 else (self.nbits // 7) >> 1


class TapChannelModel:
    """One channel of a tapped receiver: the gate of afsk_live_push over the stream's whole 2048-sample blocks
    (discard one block, wait for amp > amp_start, record through the first amp < amp_end), every recorded block fed to
    a TapDemodModel, and per push the tap outputs."""

    def __init__(self, bf: int, amp_start: int = 18000, amp_end: int = 14000, max_payload_len: int = 256):
        self.bf, self.amp_start, self.amp_end, self.max_payload = bf, amp_start, amp_end, max_payload_len
        self.reset()

    def reset(self) -> None:
        self.pos = 0
        self.carry = np.zeros(0, np.int16)
        self.mode = 0
        self.rec_start = 0
        self.dm = None

    def push(self, chunk, flush: bool = False) -> dict:
        """Returns dict(tap=bytes, tap_len=[per reported burst], bursts=[(start, length, nbytes)], open_start,
        open_nbytes) of this push."""
        data = np.concatenate([self.carry, np.asarray(chunk, np.int16)])
        base = self.pos - self.carry.size
        tap, tap_len, bursts = bytearray(), [], []
        mark = 0
        nblk = data.size // BLOCK
        for b in range(nblk):
            blk = data[b * BLOCK:(b + 1) * BLOCK]
            amp = int(np.abs(blk.astype(np.int64)).sum()) >> 11
            rec = close = False
            if self.mode == 0:
                self.mode = 1
            elif self.mode == 1:
                if amp > self.amp_start:
                    self.mode = 2
                    self.rec_start = base + b * BLOCK
                    self.dm = TapDemodModel(self.bf, self.amp_end, self.max_payload)
                    rec = True
            else:
                rec, close = True, amp < self.amp_end
            if rec:
                tap += self.dm.feed(blk)
            if close:
                bursts.append((self.rec_start, self.dm.length, self.dm.nbytes()))
                tap_len.append(len(tap) - mark)
                mark = len(tap)
                self.mode = 0
        if flush:
            if self.mode == 2:
                bursts.append((self.rec_start, self.dm.length, self.dm.nbytes()))
                tap_len.append(len(tap) - mark)
            self.reset()
        else:
            self.carry = data[nblk * BLOCK:]
            self.pos += np.asarray(chunk).size
        is_open = self.mode == 2
        return dict(tap=bytes(tap), tap_len=tap_len, bursts=bursts, open_start=self.rec_start if is_open else -1,
                    open_nbytes=self.dm.nbytes() if is_open else 0)
