"""The numpy model of the live medium's rule (include/afsk_amd.h, afsk_live_mix), for tests/test_live_mix_host.py and
tests/test_gpu_live_mix.py.  Not a test module.

``mix`` is the header's rule line by line, table clamps included: it takes the CSR arrays as they lie on the device,
so a deliberately broken table has a defined expected result.  Noise comes from the oracle's generator
(``oracle.afsk_oracle.add_noise``) run on ``pos`` zeros followed by the mixed row, then sliced -- the header's definition.
``noise_direct`` restates the header's formula in numpy for positions the oracle cannot be run up to (``pos`` near 2^32);
tests/test_live_mix_host.py holds the two against each other where both run."""
import numpy as np

from oracle import afsk_oracle as O

UNITY = 32768
MAX_GAIN = 65535
MAX_DEGREE = 32768
ORACLE_MAX_POS = 1 << 16                     # positions up to here go through the oracle


def torch_style(rows) -> np.ndarray:
    """``a.to(int32) + b.to(int32) + ...`` -> clamp -> int16: the expression the tests mixed with before."""
    total = np.sum([np.asarray(r, np.int32) for r in rows], axis=0, dtype=np.int32)
    return np.clip(total, -32768, 32767).astype(np.int16)


def _hash32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def noise_direct(row: np.ndarray, seed: int, stream_idx: int, scale_q24: int, pos: int) -> np.ndarray:
    """afsk_add_noise_batch's formula for the samples of ``row`` at sample indices (uint32)(pos + j)."""
    with np.errstate(over="ignore"):
        key = _hash32(np.uint32(seed & 0xFFFFFFFF) ^ _hash32(np.asarray([(stream_idx + 0x9e3779b9) & 0xFFFFFFFF], np.uint32)))
        t = ((pos + np.arange(row.size, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)
        total = np.zeros(row.size, np.int64)
        for k in range(8):
            h = _hash32(key ^ (t * np.uint32(8) + np.uint32(k)))
            total += (h & np.uint32(0xffff)).astype(np.int64) + (h >> np.uint32(16)).astype(np.int64)
    noise = ((total - 524280) * int(scale_q24) + (1 << 23)) >> 24
    return np.clip(row.astype(np.int64) + noise, -32768, 32767).astype(np.int16)


def noise_row(row: np.ndarray, seed: int, stream_idx: int, scale_q24: int, pos: int) -> np.ndarray:
    """``row`` as samples [pos, pos + len) of noise stream ``stream_idx``."""
    if scale_q24 == 0:
        return row.copy()
    if pos > ORACLE_MAX_POS:
        return noise_direct(row, seed, stream_idx, scale_q24, pos)
    padded = np.concatenate([np.zeros(pos, np.int16), np.asarray(row, np.int16)])
    return O.add_noise(padded, seed, stream_idx, int(scale_q24))[pos:]


def mix(src, row_ptr, link_src, link_gain_q15, n_out: int, T: int, src_lens=None, noise_scale_q24=None,
        seed: int = 0, noise_idx_base: int = 0, pos: int = 0) -> np.ndarray:
    """[n_out, T] int16: the rule over ``src`` ([n_src, >= T] int16; columns at or beyond a source's length are never
    looked at)."""
    src = np.asarray(src)
    n_src = src.shape[0]
    row_ptr, link_src, link_gain_q15 = (np.asarray(a, np.int64) for a in (row_ptr, link_src, link_gain_q15))
    n_links = link_src.size
    out = np.zeros((n_out, T), np.int16)
    for r in range(n_out):
        lo = int(np.clip(row_ptr[r], 0, n_links))
        hi = int(np.clip(row_ptr[r + 1], lo, min(n_links, lo + MAX_DEGREE)))
        acc = np.zeros(T, np.int64)
        for k in range(lo, hi):
            s = int(link_src[k])
            if not 0 <= s < n_src:
                continue
            g = int(np.clip(link_gain_q15[k], -MAX_GAIN, MAX_GAIN))
            ln = T if src_lens is None else int(np.clip(src_lens[s], 0, T))
            acc[:ln] += (g * src[s, :ln].astype(np.int64)) >> 15
            assert np.abs(acc).max(initial=0) < 2 ** 31
        row = np.clip(acc, -32768, 32767).astype(np.int16)
        if noise_scale_q24 is not None:
            row = noise_row(row, seed, (noise_idx_base + r) & 0xFFFFFFFF, int(noise_scale_q24[r]), pos)
        out[r] = row
    return out
