// afsk_live_delay.hip -- the delayed live medium (afsk_live_mix_delayed, afsk_live_mix_delayed_check,
// include/afsk_amd.h): afsk_live_mix with a delay in samples per link.  A source row is one signal over medium time;
// what it held during earlier mixes is kept on the device, in a ring of hist_len (a power of two) samples per source:
// the sample of medium time t lies at history[s][t & (hist_len - 1)].
//
// A call is three launches, in order on the caller's stream:
//   live_mix_delay_kernel    live_mix_kernel's shape -- one block per (output row, tile of kMixTile columns), one thread
//                            per 8 consecutive columns, the row's link range and every link's source, gain, length and
//                            delay the same in all lanes (scalar loads, a scalar link loop).  A link at delay d reads
//                            the 8 source columns c0 = j0 - d ... c0 + 7: wholly inside src below the source's length
//                            they are one 16-byte load at a 2-byte-aligned address, wholly inside the history without
//                            crossing the ring's end one 16-byte load from the ring, and one sample at a time where
//                            they straddle column 0, the length or the ring's end -- the threads around column d of a
//                            link and around the ring's end.  The ring is indexed with the low 32 bits of pos and a
//                            mask.  Clip, noise and the store are live_mix_kernel's.
//   live_mix_history_kernel  one block per (source row, tile of kMixTile of the columns [max(0, T - hist_len), T)):
//                            history[s][(pos + j) & mask] = j < len_s ? src[s][j] : 0, 8 columns per thread as one
//                            16-byte load and one 16-byte store where they neither straddle the length nor the ring's
//                            end.  It runs behind the mix, which has read the slots it overwrites: a delay of hist_len
//                            is legal.
//   live_mix_advance_kernel  afsk_live_mix.hip's: *pos += T.
// Nothing is read through a table entry before it was clamped: what live_mix_kernel clamps, and a delay to
// [0, hist_len]; a link whose source lies outside the matrix reads neither src nor the history.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end), behind
// afsk_live_mix.hip, whose constants, MixArgs and advance kernel it uses.

namespace afsk {

constexpr int32_t kMixMinHist = 8;
constexpr int32_t kMixMaxHist = 1 << 20;

struct MixDelayArgs {
    MixArgs m;
    int32_t hist_len;               // a power of two in kMixMinHist ... kMixMaxHist
    int32_t first;                  // the history kernel: the first column it writes, max(0, T - hist_len)
};

__device__ __forceinline__ void mix_add8(int32_t (&acc)[8], int32_t g, const store16 w) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        acc[2 * d] += __mul24(g, (int32_t)(int16_t)(w[d] & 0xffffu)) >> 15;
        acc[2 * d + 1] += __mul24(g, (int32_t)w[d] >> 16) >> 15;
    }
}

__global__ __launch_bounds__(kMixThreads) void live_mix_delay_kernel(MixDelayArgs da, const int16_t* __restrict__ src,
                                                                     const int32_t* __restrict__ src_lens,
                                                                     const int32_t* __restrict__ row_ptr,
                                                                     const int32_t* __restrict__ link_src,
                                                                     const int32_t* __restrict__ link_gain,
                                                                     const int32_t* __restrict__ link_delay,
                                                                     const int16_t* __restrict__ history,
                                                                     const int32_t* __restrict__ noise_scale,
                                                                     const int64_t* __restrict__ pos_ptr) {
    const MixArgs& a = da.m;
    const int32_t bid = xcd_block((int)blockIdx.x, (int)gridDim.x);
    const int32_t r = bid / a.tiles;
    const int32_t tile = bid - r * a.tiles;
    const int32_t T = a.n_samples;
    const int32_t j0 = tile * kMixTile + (int32_t)threadIdx.x * 8;
    if (j0 >= T) return;
    const uint32_t pos32 = (uint32_t)(uint64_t)*pos_ptr;
    const uint32_t mask = (uint32_t)da.hist_len - 1u;
    const int32_t lo = min(max(row_ptr[r], 0), a.n_links);
    const int32_t hi = min(max(row_ptr[r + 1], lo), lo + min(a.n_links - lo, kMixMaxDegree));
    int32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t k = lo; k < hi; k++) {
        const int32_t s = link_src[k];
        if ((uint32_t)s >= (uint32_t)a.n_src) continue;           // a source outside the matrix is silent
        const int32_t g = min(max(link_gain[k], -kMixMaxGain), kMixMaxGain);
        const int32_t d = min(max(link_delay[k], 0), da.hist_len);
        const int32_t len = src_lens ? min(max(src_lens[s], 0), T) : T;
        const int32_t c0 = j0 - d;                                // in [-hist_len, T)
        if (c0 >= len) continue;
        const int16_t* p = src + (int64_t)s * a.src_stride;
        const int16_t* ring = history + (int64_t)s * da.hist_len;
        const uint32_t h0 = (pos32 + (uint32_t)c0) & mask;        // the ring slot of column c0 (c0 < 0: an earlier mix)
        if (c0 >= 0 && c0 + 8 <= len) {
            mix_add8(acc, g, *reinterpret_cast<const store16*>(p + c0));
        } else if (c0 + 8 <= 0 && h0 + 8u <= (uint32_t)da.hist_len) {
            mix_add8(acc, g, *reinterpret_cast<const store16*>(ring + h0));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int32_t c = c0 + j;
                if (c < 0)
                    acc[j] += __mul24(g, (int32_t)ring[(h0 + (uint32_t)j) & mask]) >> 15;
                else if (c < len)
                    acc[j] += __mul24(g, (int32_t)p[c]) >> 15;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = min(max(acc[j], -32768), 32767);
    const int32_t scale = noise_scale ? noise_scale[r] : 0;
    if (scale != 0) {                                             // per row: block-uniform
        const uint32_t key = noise_key(a.noise_seed, a.noise_idx_base + (uint32_t)r);
        const uint32_t t0 = pos32 + (uint32_t)j0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j0 + j < T) {
                const int64_t v = (int64_t)acc[j] + noise_term(key, t0 + (uint32_t)j, scale);
                acc[j] = (int32_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
            }
    }
    int16_t* dst = a.out + (int64_t)r * a.out_stride + j0;
    if (j0 + 8 <= T) {
        store16 w;
#pragma unroll
        for (int d = 0; d < 4; d++) w[d] = ((uint32_t)acc[2 * d] & 0xffffu) | ((uint32_t)acc[2 * d + 1] << 16);
        *reinterpret_cast<store16*>(dst) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j0 + j < T) dst[j] = (int16_t)acc[j];
    }
}

__global__ __launch_bounds__(kMixThreads) void live_mix_history_kernel(MixDelayArgs da, const int16_t* __restrict__ src,
                                                                       const int32_t* __restrict__ src_lens,
                                                                       int16_t* __restrict__ history,
                                                                       const int64_t* __restrict__ pos_ptr) {
    const MixArgs& a = da.m;
    const int32_t bid = (int32_t)blockIdx.x;
    const int32_t s = bid / a.tiles;                              // (tiles: of the columns this kernel writes)
    const int32_t tile = bid - s * a.tiles;
    const int32_t T = a.n_samples;
    const int32_t j0 = da.first + tile * kMixTile + (int32_t)threadIdx.x * 8;
    if (j0 >= T) return;
    const uint32_t mask = (uint32_t)da.hist_len - 1u;
    const uint32_t h0 = ((uint32_t)(uint64_t)*pos_ptr + (uint32_t)j0) & mask;
    const int32_t len = src_lens ? min(max(src_lens[s], 0), T) : T;
    const int16_t* p = src + (int64_t)s * a.src_stride + j0;
    int16_t* ring = history + (int64_t)s * da.hist_len;
    if (j0 + 8 <= T && h0 + 8u <= (uint32_t)da.hist_len && (j0 + 8 <= len || j0 >= len)) {
        store16 w = store16{0u, 0u, 0u, 0u};
        if (j0 < len) w = *reinterpret_cast<const store16*>(p);
        *reinterpret_cast<store16*>(ring + h0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j0 + j < T) ring[(h0 + (uint32_t)j) & mask] = j0 + j < len ? p[j] : (int16_t)0;
    }
}

inline bool mix_hist_len_valid(int32_t hist_len) {
    return hist_len >= kMixMinHist && hist_len <= kMixMaxHist && (hist_len & (hist_len - 1)) == 0;
}

}  // namespace afsk

extern "C" {

int afsk_live_mix_delayed_check(const int32_t* h_row_ptr, const int32_t* h_link_src, const int32_t* h_link_gain_q15,
                                const int32_t* h_link_delay, int32_t n_out, int32_t n_src, int32_t n_links,
                                int32_t hist_len) {
    if (!afsk::mix_hist_len_valid(hist_len))
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_delayed_check: hist_len must be a power of two in 8 ... 2^20");
    if (n_links > 0 && !h_link_delay)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_delayed_check: null link_delay");
    if (int rc = afsk_live_mix_check(h_row_ptr, h_link_src, h_link_gain_q15, n_out, n_src, n_links)) return rc;
    return afsk::no_throw([&] {
        for (int32_t k = 0; k < n_links; k++)
            if (h_link_delay[k] < 0 || h_link_delay[k] > hist_len)
                return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_delayed_check: link " + std::to_string(k) +
                                                          " has a delay of " + std::to_string(h_link_delay[k]) +
                                                          " outside 0 ... hist_len = " + std::to_string(hist_len));
        return (int)AFSK_OK;
    });
}

int afsk_live_mix_delayed(const int16_t* src, int64_t src_row_stride, int32_t n_src, const int32_t* d_src_lens_or_null,
                          const int32_t* d_row_ptr, const int32_t* d_link_src, const int32_t* d_link_gain_q15,
                          const int32_t* d_link_delay, int32_t n_links, int16_t* out, int64_t out_row_stride,
                          int32_t n_out, int32_t n_samples, const int32_t* d_noise_scale_q24_or_null,
                          uint32_t noise_seed, uint32_t noise_idx_base, int64_t* d_pos, int16_t* d_history,
                          int32_t hist_len, void* hip_stream) {
    const char* const me = "afsk_live_mix_delayed: ";
    auto bad = [&](const char* what) { return afsk::fail(AFSK_E_INVALID_ARG, std::string(me) + what); };
    if (n_src < 0 || n_links < 0 || n_out < 0) return bad("negative count");
    if (n_samples < 0 || n_samples > afsk::kMixMaxSamples) return bad("n_samples must lie in 0 ... 2^20");
    if (!afsk::mix_hist_len_valid(hist_len)) return bad("hist_len must be a power of two in 8 ... 2^20");
    if ((n_src > 0 && (!src || !d_history)) || (n_out > 0 && (!out || !d_row_ptr)) ||
        (n_links > 0 && (!d_link_src || !d_link_gain_q15 || !d_link_delay)) || !d_pos)
        return bad("null pointer argument");
    if ((n_src > 1 && src_row_stride < n_samples) || (n_out > 1 && out_row_stride < n_samples))
        return bad("a row stride below n_samples (rows would overlap)");
    if (n_src > 0 && n_samples > 0) {
        // the bytes the kernels may touch: columns [0, n_samples) of every row, and the whole history
        const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out, h0 = (uintptr_t)d_history;
        const uintptr_t s1 = s0 + 2 * ((uintptr_t)(n_src - 1) * (uintptr_t)(n_src > 1 ? src_row_stride : 0) + n_samples);
        const uintptr_t o1 = o0 + 2 * ((uintptr_t)(n_out > 0 ? n_out - 1 : 0) * (uintptr_t)(n_out > 1 ? out_row_stride : 0) + n_samples);
        const uintptr_t h1 = h0 + 2 * (uintptr_t)n_src * (uintptr_t)hist_len;
        if (n_out > 0 && s0 < o1 && o0 < s1) return bad("out overlaps src");
        if (s0 < h1 && h0 < s1) return bad("the history overlaps src");
        if (n_out > 0 && o0 < h1 && h0 < o1) return bad("the history overlaps out");
    }
    if (n_samples == 0 || n_out == 0) return AFSK_OK;
    afsk::MixDelayArgs a{};
    a.m.out = out;
    a.m.out_stride = n_out > 1 ? out_row_stride : 0;
    a.m.src_stride = n_src > 1 ? src_row_stride : 0;
    a.m.n_src = n_src;
    a.m.n_links = n_links;
    a.m.n_samples = n_samples;
    a.m.tiles = (n_samples + afsk::kMixTile - 1) / afsk::kMixTile;
    a.m.noise_seed = noise_seed;
    a.m.noise_idx_base = noise_idx_base;
    a.hist_len = hist_len;
    afsk::MixDelayArgs h = a;                                     // the history kernel's: its own columns and tiles
    h.first = n_samples > hist_len ? n_samples - hist_len : 0;
    h.m.tiles = (n_samples - h.first + afsk::kMixTile - 1) / afsk::kMixTile;
    const int64_t blocks = (int64_t)a.m.tiles * n_out, hblocks = (int64_t)h.m.tiles * n_src;
    if (blocks > 0x7fffffffll) return bad("n_out * tiles exceeds 2^31 - 1");
    if (hblocks > 0x7fffffffll) return bad("n_src * tiles of the history exceeds 2^31 - 1");
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_mix_delay_kernel, dim3((uint32_t)blocks), dim3(afsk::kMixThreads), 0, st, a, src,
                       d_src_lens_or_null, d_row_ptr, d_link_src, d_link_gain_q15, d_link_delay,
                       (const int16_t*)d_history, d_noise_scale_q24_or_null, (const int64_t*)d_pos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_delay_kernel");
    if (hblocks > 0) {                                            // (no sources: no history to write)
        hipLaunchKernelGGL(afsk::live_mix_history_kernel, dim3((uint32_t)hblocks), dim3(afsk::kMixThreads), 0, st, h,
                           src, d_src_lens_or_null, d_history, (const int64_t*)d_pos);
        e = hipGetLastError();
        if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_history_kernel");
    }
    hipLaunchKernelGGL(afsk::live_mix_advance_kernel, dim3(1), dim3(1), 0, st, d_pos, n_samples);
    e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_advance_kernel");
    return AFSK_OK;
}

}  // extern "C"
