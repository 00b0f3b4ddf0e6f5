"""The numpy model of the delayed live medium's rule (include/afsk_amd.h, afsk_live_mix_delayed), for
tests/test_live_delay_host.py and tests/test_gpu_live_delay.py.  Not a test module.

``Timeline`` keeps every source row as ONE signal over medium time, whole: ``X[s, i]`` is what source s held at time
``start + i``, a column at or beyond a mix's length is 0, and a time before ``start`` is 0.  Nothing in it is a ring:
``hist_len`` appears only as the bound a delay is clamped to.  Gains, the table clamps, the clip and the noise are
tests/live_mix_model.py's; the tables are passed to every mix as they lie on the device, so a deliberately broken
table has a defined expected result."""
import numpy as np

from tests import live_mix_model as M


class Timeline:
    def __init__(self, n_src: int, hist_len: int, pos: int = 0):
        self.n_src, self.hist_len, self.start = int(n_src), int(hist_len), int(pos)
        self.X = np.zeros((self.n_src, 0), np.int16)

    @property
    def pos(self) -> int:
        return self.start + self.X.shape[1]

    def mix(self, src, row_ptr, link_src, link_gain_q15, link_delay, n_out: int, T: int, src_lens=None,
            noise_scale_q24=None, seed: int = 0, noise_idx_base: int = 0) -> np.ndarray:
        """[n_out, T] int16: the mix of columns [0, T) of ``src`` at the timeline's position, which it then advances."""
        src = np.asarray(src)
        assert src.shape[0] == self.n_src
        pos, before = self.pos, self.X.shape[1]
        cur = np.zeros((self.n_src, T), np.int16)
        for s in range(self.n_src):
            ln = T if src_lens is None else int(np.clip(src_lens[s], 0, T))
            cur[s, :ln] = src[s, :ln]
        X = np.concatenate([self.X, cur], axis=1)
        row_ptr, link_src, link_gain_q15, link_delay = (np.asarray(a, np.int64) for a in
                                                        (row_ptr, link_src, link_gain_q15, link_delay))
        n_links = link_src.size
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
                d = int(np.clip(link_delay[k], 0, self.hist_len))
                at = before + np.arange(T, dtype=np.int64) - d           # X's column of time pos + j - d
                x = np.where(at >= 0, X[s, np.maximum(at, 0)], 0).astype(np.int64)
                acc += (g * x) >> 15
                assert np.abs(acc).max(initial=0) < 2 ** 31
            row = np.clip(acc, -32768, 32767).astype(np.int16)
            if noise_scale_q24 is not None:
                row = M.noise_row(row, seed, (noise_idx_base + r) & 0xFFFFFFFF, int(noise_scale_q24[r]), pos)
            out[r] = row
        self.X = X
        return out
