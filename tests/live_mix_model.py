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


# ------------------------------------------------------------------------------------- tables at the header's limits

def limit_links():
    """``(n_src, n_out, links)``: source 0 is to be held at -32768, source 1 is any.  Row 0: MAX_DEGREE links at gain
    -MAX_GAIN on source 0 -- 32768 * 65535 = 2147450880, the bound the header gives for a row's int32 sum.  Row 1, of
    MAX_DEGREE links too: 16383 such links, 16383 at +MAX_GAIN on the same source, one unity link to source 1 and one
    of gain 0 -- the sum climbs to 1073659905, comes back to 0 and ends as source 1's sample, unless something wrapped or
    saturated on the way.  (16384 of each and the unity link would be 32769 links: one more than a row may have.)"""
    half = MAX_DEGREE // 2 - 1
    links = [(0, 0, -MAX_GAIN)] * MAX_DEGREE + [(1, 0, -MAX_GAIN)] * half + [(1, 0, MAX_GAIN)] * half + \
        [(1, 1, UNITY), (1, 0, 0)]
    return 2, 2, links


SPAN_TAIL = 7400                             # links of row 1 in ``span_links``: row_ptr[1] = 40000 stays inside them


def span_links():
    """``(n_src, n_out, links)`` for a ``row_ptr`` span above MAX_DEGREE written onto the device: row 0 holds exactly
    MAX_DEGREE links whose sum is source 1's sample (a unity link, 16383 pairs of +-unity on source 2 that cancel, a
    link of gain 0), row 1 the ``SPAN_TAIL`` links that follow them in the arrays, a quarter of source 3 each.  With
    ``row_ptr[1]`` raised to 32769 or 40000 every index up to it names a real link, so a missing clamp to MAX_DEGREE
    links shows as source 3 in row 0's sum -- never as a read outside the arrays."""
    row0 = [(0, 1, UNITY)] + [(0, 2, UNITY), (0, 2, -UNITY)] * (MAX_DEGREE // 2 - 1) + [(0, 2, 0)]
    assert len(row0) == MAX_DEGREE
    return 4, 2, row0 + [(1, 3, UNITY // 4)] * SPAN_TAIL
