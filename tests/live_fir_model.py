"""The numpy model of the filtered live medium's rule (include/afsk_amd.h, afsk_live_mix_filtered), for
tests/test_live_fir_host.py, tests/test_live_fir_stub.py and tests/test_gpu_live_fir.py.  Not a test module.

``Timeline`` is tests/live_delay_model.py's -- every source row ONE signal over medium time, nothing in it a ring --
with the filtered link's rule: ``v = sum_i h[i] * x[t - d - i]`` in int64 (asserted to fit int32), ``f = clamp(v >> 14)``,
``(g * f) >> 15``.  The tables are passed to every mix as they lie on the device, with the device's clamps, so a
deliberately broken table has a defined expected result."""
import numpy as np

from tests import live_delay_model as D
from tests import live_mix_model as M

MAX_TAPS = 256
MAX_L1 = 65535
Q14 = 16384


def design(n_taps: int, low_hz: float = 0, high_hz=None, rate: int = 48000) -> list:
    """The Hamming windowed sinc in Q14, written out independently of ``live.fir_design``."""
    high_hz = rate / 2 if high_hz is None else high_hz
    m = np.arange(n_taps) - (n_taps - 1) / 2
    h = 2 * high_hz / rate * np.sinc(2 * high_hz / rate * m)
    if low_hz > 0:
        h = h - 2 * low_hz / rate * np.sinc(2 * low_hz / rate * m)
    return [int(v) for v in np.round(h * np.hamming(n_taps) * Q14)]


class Timeline(D.Timeline):
    def mix(self, src, row_ptr, link_src, link_gain_q15, link_delay, n_out: int, T: int, src_lens=None,
            noise_scale_q24=None, seed: int = 0, noise_idx_base: int = 0, link_filter=None, filter_ptr=(0,),
            filter_taps=()) -> np.ndarray:
        """[n_out, T] int16: the mix of columns [0, T) of ``src`` at the timeline's position, which it then advances.
        ``link_filter`` None: every link is unfiltered (the delayed model)."""
        src = np.asarray(src)
        assert src.shape[0] == self.n_src
        pos, before = self.pos, self.X.shape[1]
        cur = np.zeros((self.n_src, T), np.int16)
        for s in range(self.n_src):
            ln = T if src_lens is None else int(np.clip(src_lens[s], 0, T))
            cur[s, :ln] = src[s, :ln]
        X = np.concatenate([self.X, cur], axis=1)
        row_ptr, link_src, link_gain_q15, link_delay, filter_ptr, taps = (
            np.asarray(a, np.int64) for a in (row_ptr, link_src, link_gain_q15, link_delay, filter_ptr, filter_taps))
        link_filter = np.full(link_src.size, -1, np.int64) if link_filter is None else np.asarray(link_filter, np.int64)
        n_links, n_filters, n_taps = link_src.size, filter_ptr.size - 1, taps.size
        t = before + np.arange(T, dtype=np.int64)                       # X's column of time pos + j

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
                f = int(link_filter[k])
                if f == -1:
                    d = int(np.clip(link_delay[k], 0, self.hist_len))
                    acc += (g * x_at(s, t - d)) >> 15
                    continue
                if not 0 <= f < n_filters:
                    continue
                t0 = int(np.clip(filter_ptr[f], 0, n_taps))
                t1 = int(np.clip(filter_ptr[f + 1], t0, n_taps))
                K = min(t1 - t0, MAX_TAPS, self.hist_len + 1)
                if K == 0:
                    continue
                d = int(np.clip(link_delay[k], 0, self.hist_len - (K - 1)))
                v = np.zeros(T, np.int64)
                for i in range(K):
                    v += int(taps[t0 + i]) * x_at(s, t - d - i)
                assert np.abs(v).max(initial=0) < 2 ** 31
                acc += (g * np.clip(v >> 14, -32768, 32767)) >> 15
                assert np.abs(acc).max(initial=0) < 2 ** 31
            row = np.clip(acc, -32768, 32767).astype(np.int16)
            if noise_scale_q24 is not None:
                row = M.noise_row(row, seed, (noise_idx_base + r) & 0xFFFFFFFF, int(noise_scale_q24[r]), pos)
            out[r] = row
        self.X = X
        return out
