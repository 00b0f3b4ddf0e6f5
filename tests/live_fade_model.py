"""The numpy model of the faded live medium's rule (include/afsk_amd.h, afsk_live_mix_faded), for
tests/test_live_fade_host.py, tests/test_live_fade_stub.py and tests/test_gpu_live_fade.py.  Not a test module.

``Timeline`` is tests/live_fir_model.py's -- every source row ONE signal over medium time, nothing in it a ring -- with
the faded link's rule between the link's sample and its gain: the envelope ``e`` of ``envelope`` below, then
``(g * clamp16((e * x) >> 15)) >> 15``, all in int64 with the int32 fits asserted.  The tables are passed to every mix as
they lie on the device, with the device's clamps, so a deliberately broken table has a defined expected result.
``design`` writes ``live.fade_design`` out independently, sinusoid by sinusoid."""
import numpy as np

from tests import live_fir_model as F
from tests import live_mix_model as M

MAX_KNOTS = 65536
MIN_SHIFT, MAX_SHIFT = 3, 15
Q15 = 32768
SPREAD = 0x9E3779B1


def envelope(knots, p: int, u) -> np.ndarray:
    """e at the uint32 track positions ``u`` (any integers: taken mod 2^32) of a track of ``len(knots)`` knots (a
    power of two) at 2^p samples per knot."""
    knots = np.asarray(knots, np.int64)
    L = knots.size
    assert L >= 1 and L & (L - 1) == 0 and MIN_SHIFT <= p <= MAX_SHIFT
    u = np.asarray(u, np.int64) & 0xFFFFFFFF
    n = (u >> p) & (L - 1)
    m = (n + 1) & (L - 1)
    q = u & ((1 << p) - 1)
    prod = (knots[m] - knots[n]) * q
    assert np.abs(prod).max(initial=0) < 2 ** 31
    e = knots[n] + (prod >> p)                                  # (numpy's >> on int64 is arithmetic: floor)
    assert e.min(initial=0) >= 0 and e.max(initial=0) <= 65535
    return e


def fade_sample(e, x) -> np.ndarray:
    prod = np.asarray(e, np.int64) * np.asarray(x, np.int64)
    assert np.abs(prod).max(initial=0) < 2 ** 31
    return np.clip(prod >> 15, -32768, 32767)


def design(n_knots: int, period: int, doppler_hz: float, k_factor=None, seed: int = 0, rate: int = 48000,
           at=None) -> list:
    """``live.fade_design``'s knots written out as a plain sum of sinusoids.  ``at``: the knot indices to evaluate
    (None: 0 ... n_knots - 1); any integer is legal, which is how the seam is looked at."""
    kmax = int(np.floor(doppler_hz * n_knots * period / rate))
    ks = list(range(-kmax, kmax + 1))
    amp = np.random.default_rng(seed).standard_normal((2, len(ks)))

    def scatter(idx):
        z = np.zeros(len(idx), np.complex128)
        for i, k in enumerate(ks):
            w = (1 - (k / (kmax + 0.5)) ** 2) ** -0.25
            ph = 2 * np.pi * k * np.asarray(idx, np.float64) / n_knots
            z += w * complex(amp[0, i], amp[1, i]) * (np.cos(ph) + 1j * np.sin(ph))
        return z
    whole = scatter(np.arange(n_knots))
    rms = np.sqrt(np.mean(np.abs(whole) ** 2))
    los = 0.0 if k_factor is None else np.sqrt(k_factor)
    rms2 = np.sqrt(np.mean(np.abs(whole / rms + los) ** 2))
    z = (scatter(np.arange(n_knots) if at is None else np.asarray(at)) / rms + los) / rms2
    return [int(v) for v in np.minimum(np.round(np.abs(z) * Q15), 65535)]


class Timeline(F.Timeline):
    def mix(self, src, row_ptr, link_src, link_gain_q15, link_delay, n_out: int, T: int, src_lens=None,
            noise_scale_q24=None, seed: int = 0, noise_idx_base: int = 0, link_filter=None, filter_ptr=(0,),
            filter_taps=(), link_fade=None, link_fade_offset=None, fade_ptr=(0,), fade_shift=(),
            fade_knots=()) -> np.ndarray:
        """[n_out, T] int16: the mix of columns [0, T) of ``src`` at the timeline's position, which it then advances.
        ``link_fade`` None: no link has a track (the filtered model)."""
        if link_fade is None:
            return super().mix(src, row_ptr, link_src, link_gain_q15, link_delay, n_out, T, src_lens, noise_scale_q24,
                               seed, noise_idx_base, link_filter, filter_ptr, filter_taps)
        src = np.asarray(src)
        assert src.shape[0] == self.n_src
        pos, before = self.pos, self.X.shape[1]
        cur = np.zeros((self.n_src, T), np.int16)
        for s in range(self.n_src):
            ln = T if src_lens is None else int(np.clip(src_lens[s], 0, T))
            cur[s, :ln] = src[s, :ln]
        X = np.concatenate([self.X, cur], axis=1)
        row_ptr, link_src, link_gain_q15, link_delay, filter_ptr, taps, link_fade, fade_ptr, fade_shift, knots = (
            np.asarray(a, np.int64) for a in (row_ptr, link_src, link_gain_q15, link_delay, filter_ptr, filter_taps,
                                              link_fade, fade_ptr, fade_shift, fade_knots))
        link_filter = np.full(link_src.size, -1, np.int64) if link_filter is None else np.asarray(link_filter, np.int64)
        link_fade_offset = np.zeros(link_src.size, np.int64) if link_fade_offset is None \
            else np.asarray(link_fade_offset, np.int64)
        n_links, n_filters, n_taps = link_src.size, filter_ptr.size - 1, taps.size
        n_fades, n_knots = fade_ptr.size - 1, knots.size
        t = before + np.arange(T, dtype=np.int64)                       # X's column of time pos + j
        now = pos + np.arange(T, dtype=np.int64)                        # the listener's time

        def x_at(s, at):
            return np.where(at >= 0, X[s, np.maximum(at, 0)], 0).astype(np.int64)

        out = np.zeros((n_out, T), np.int16)
        for r in range(n_out):
            lo = int(np.clip(row_ptr[r], 0, n_links))
            hi = int(np.clip(row_ptr[r + 1], lo, min(n_links, lo + M.MAX_DEGREE)))
            acc = np.zeros(T, np.int64)
            for k in range(lo, hi):
                s = int(link_src[k])
                if not 0 <= s < self.n_src:
                    continue
                g = int(np.clip(link_gain_q15[k], -M.MAX_GAIN, M.MAX_GAIN))
                fd = int(link_fade[k])
                e = None
                if fd != -1:
                    if not 0 <= fd < n_fades:
                        continue
                    q0 = int(np.clip(fade_ptr[fd], 0, n_knots))
                    q1 = int(np.clip(fade_ptr[fd + 1], q0, n_knots))
                    n = min(q1 - q0, MAX_KNOTS)
                    if n == 0:
                        continue
                    L = 1 << (n.bit_length() - 1)
                    p = int(np.clip(fade_shift[fd], MIN_SHIFT, MAX_SHIFT))
                    e = envelope(knots[q0:q0 + L], p, now + int(link_fade_offset[k]))
                f = int(link_filter[k])
                if f == -1:
                    d = int(np.clip(link_delay[k], 0, self.hist_len))
                    x = x_at(s, t - d)
                else:
                    if not 0 <= f < n_filters:
                        continue
                    t0 = int(np.clip(filter_ptr[f], 0, n_taps))
                    t1 = int(np.clip(filter_ptr[f + 1], t0, n_taps))
                    K = min(t1 - t0, F.MAX_TAPS, self.hist_len + 1)
                    if K == 0:
                        continue
                    d = int(np.clip(link_delay[k], 0, self.hist_len - (K - 1)))
                    v = np.zeros(T, np.int64)
                    for i in range(K):
                        v += int(taps[t0 + i]) * x_at(s, t - d - i)
                    assert np.abs(v).max(initial=0) < 2 ** 31
                    x = np.clip(v >> 14, -32768, 32767)
                if e is not None:
                    x = fade_sample(e, x)
                acc += (g * x) >> 15
                assert np.abs(acc).max(initial=0) < 2 ** 31
            row = np.clip(acc, -32768, 32767).astype(np.int16)
            if noise_scale_q24 is not None:
                row = M.noise_row(row, seed, (noise_idx_base + r) & 0xFFFFFFFF, int(noise_scale_q24[r]), pos)
            out[r] = row
        self.X = X
        return out
