// afsk_live_fir.hip -- the filtered live medium (afsk_live_mix_filtered, afsk_live_mix_filtered_check,
// include/afsk_amd.h): afsk_live_mix_delayed with an FIR filter in Q14 taps per link.  A link with filter h (K taps),
// delay d and gain g contributes (g * clamp((sum_i h[i] * x_s[t - d - i]) >> 14)) >> 15 at medium time t; x_s is the
// delayed medium's timeline unchanged (src below the source's length, 0 beyond, the history ring before pos).
//
// A call is three launches, in order on the caller's stream:
//   live_mix_fir_kernel      live_mix_delay_kernel's shape -- one block per (output row, tile of kMixTile columns), one
//                            thread per 8 consecutive columns, a scalar link loop.  A link without a filter takes that
//                            kernel's three-way path.  For a link with one the block first stages, once, the
//                            kMixTile + Kp timeline samples its tile needs into LDS (Kp: K rounded up to kFirChunk):
//                              win[i] = x_s[tile0 - d - (K - 1) + i]
//                            every group of 8 decided like the delay kernel decides its 8 columns (one 16-byte load
//                            from src, one from the ring, zeros, or one sample at a time at an edge; fir_group_addr,
//                            fir_group_edge: a thread's loads are all issued before it waits for one), and the taps,
//                            reversed and zero-padded (g[q] = h[K - 1 - q]), in the two packings the two output
//                            parities need:
//                              tap_even[m] = (g[2m], g[2m + 1])        column j even: sum_m dot2(win word j/2 + m, .)
//                              tap_odd[m]  = (g[2m - 1], g[2m])        column j odd:  sum_m dot2(win word (j-1)/2 + m, .)
//                            with g[-1] = g[Kp] = 0, so no lane ever realigns a sample: every dot2 takes an aligned
//                            32-bit word of win.  A thread then walks the taps kFirChunk at a time: 3 ds_read_b128 of
//                            samples (8 + 16), 4 ds_read_b128 of packed taps at an address all lanes share, 64
//                            v_dot2c_i32_i16 (__builtin_amdgcn_sdot2, no clamp: the sum wraps like the rule's int32).
//                            tap_odd has one word more than tap_even; it is non-zero only when
//                            K == Kp and costs one more read and 4 dot2 then.  The multiply loop has no edge cases.
//                            (The taps are int16 at a 2-byte-aligned address: they cannot arrive as scalar dword
//                            loads without demanding more of the table, so they take the LDS broadcast path.)
//                            Threads beyond column T stage like the others and leave behind the last barrier; the
//                            link loop is block-uniform, so the barriers inside it are legal.
//   live_mix_history_kernel  afsk_live_delay.hip's, unchanged.
//   live_mix_advance_kernel  afsk_live_mix.hip's.
// Nothing is read through a table entry before it was clamped: what live_mix_delay_kernel clamps; a filter index
// outside -1 ... n_filters - 1 is silent; filter_ptr entries to [0, n_taps]; K to 0 ... min(kFirMaxTaps, hist_len + 1),
// K = 0 silent; the delay to [0, hist_len - (K - 1)], so the reach d + K - 1 stays within the history.  Taps are values,
// not addresses: a table whose sum |h| exceeds 65535 (refused by the check) may wrap the 32-bit sum, nothing else.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end), behind
// afsk_live_delay.hip, whose MixDelayArgs, mix_add8 and history kernel it uses.

namespace afsk {

constexpr int32_t kFirMaxTaps = 256;
constexpr int32_t kFirChunk = 16;                               // taps per step of the multiply loop
constexpr int32_t kFirMaxL1 = 65535;                            // sum |h|: 65535 * 32768 < 2^31
constexpr int32_t kFirWin = kMixTile + kFirMaxTaps;             // staged samples
constexpr int32_t kFirTapWords = kFirMaxTaps / 2 + 8;           // packed tap words of one parity (odd: one more, padded)

typedef short fir_s16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t fir_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int32_t fir_dot2(uint32_t pair, uint32_t coef, int32_t acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(fir_s16x2, pair), __builtin_bit_cast(fir_s16x2, coef), acc, false);
}

// Staging the 8 timeline samples of columns c0 ... c0 + 7 of one source (c0 >= -hist_len; p: its src row, ring: its history
// row) is split in two, so that a thread has all its loads in flight before it waits for any -- the whole block waits
// for the slowest thread at the barrier.  fir_group_addr: where the 8 samples lie as ONE 16-byte load, `whole` when they
// do -- wholly inside src below the length, or wholly inside the history without crossing the ring's end; otherwise the
// ring's first 8 slots, always readable, whose value is not used.  fir_group_edge, for a group that is not whole: zeros
// at or beyond the length; with column 0, the length or the ring's end inside the 8, every sample by a selected address
// (eight loads in flight together; a column at or beyond the length loads its ring slot and counts as 0).
__device__ __forceinline__ const int16_t* fir_group_addr(const int16_t* __restrict__ p, const int16_t* __restrict__ ring,
                                                         int32_t c0, int32_t len, uint32_t pos32, uint32_t mask,
                                                         bool& whole) {
    const uint32_t h0 = (pos32 + (uint32_t)c0) & mask;            // the ring slot of column c0
    const bool in_src = c0 >= 0 && c0 + 8 <= len;
    const bool in_ring = c0 + 8 <= 0 && h0 + 8u <= mask + 1u;
    whole = in_src || in_ring;
    return in_src ? p + c0 : ring + (in_ring ? h0 : 0u);
}

__device__ __forceinline__ store16 fir_group_edge(const int16_t* __restrict__ p, const int16_t* __restrict__ ring,
                                                  int32_t c0, int32_t len, uint32_t pos32, uint32_t mask) {
    store16 w = store16{0u, 0u, 0u, 0u};
    if (c0 < len) {
        const uint32_t h0 = (pos32 + (uint32_t)c0) & mask;
        uint32_t x[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int32_t c = c0 + j;
            const int16_t* q = (c >= 0 && c < len) ? p + c : ring + ((h0 + (uint32_t)j) & mask);
            const int16_t v = *q;
            x[j] = c < len ? (uint32_t)(uint16_t)v : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) w[q] = x[2 * q] | (x[2 * q + 1] << 16);
    }
    return w;
}

struct MixFirArgs {
    MixDelayArgs d;
    int32_t n_filters;
    int32_t n_taps;                 // entries of filter_taps
};

__global__ __launch_bounds__(kMixThreads) void live_mix_fir_kernel(MixFirArgs fa, const int16_t* __restrict__ src,
                                                                   const int32_t* __restrict__ src_lens,
                                                                   const int32_t* __restrict__ row_ptr,
                                                                   const int32_t* __restrict__ link_src,
                                                                   const int32_t* __restrict__ link_gain,
                                                                   const int32_t* __restrict__ link_delay,
                                                                   const int32_t* __restrict__ link_filter,
                                                                   const int32_t* __restrict__ filter_ptr,
                                                                   const int16_t* __restrict__ filter_taps,
                                                                   const int16_t* __restrict__ history,
                                                                   const int32_t* __restrict__ noise_scale,
                                                                   const int64_t* __restrict__ pos_ptr) {
    __shared__ __attribute__((aligned(16))) int16_t win[kFirWin];
    __shared__ __attribute__((aligned(16))) uint32_t tap_even[kFirTapWords];
    __shared__ __attribute__((aligned(16))) uint32_t tap_odd[kFirTapWords];
    const MixDelayArgs& da = fa.d;
    const MixArgs& a = da.m;
    const int32_t bid = xcd_block((int)blockIdx.x, (int)gridDim.x);
    const int32_t r = bid / a.tiles;
    const int32_t tile = bid - r * a.tiles;
    const int32_t T = a.n_samples;
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t tile0 = tile * kMixTile;
    const int32_t j0 = tile0 + tid * 8;
    const bool live = j0 < T;                                     // (a thread beyond column T still stages)
    const uint32_t pos32 = (uint32_t)(uint64_t)*pos_ptr;
    const uint32_t mask = (uint32_t)da.hist_len - 1u;
    const int32_t lo = min(max(row_ptr[r], 0), a.n_links);
    const int32_t hi = min(max(row_ptr[r + 1], lo), lo + min(a.n_links - lo, kMixMaxDegree));
    int32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool staged = false;                                          // block-uniform: win and the taps hold a link's
    for (int32_t k = lo; k < hi; k++) {
        const int32_t s = link_src[k];
        if ((uint32_t)s >= (uint32_t)a.n_src) continue;           // a source outside the matrix is silent
        const int32_t g = min(max(link_gain[k], -kMixMaxGain), kMixMaxGain);
        const int32_t len = src_lens ? min(max(src_lens[s], 0), T) : T;
        const int16_t* p = src + (int64_t)s * a.src_stride;
        const int16_t* ring = history + (int64_t)s * da.hist_len;
        const int32_t f = link_filter[k];
        if (f == -1) {                                            // live_mix_delay_kernel's link
            if (!live) continue;
            const int32_t d = min(max(link_delay[k], 0), da.hist_len);
            const int32_t c0 = j0 - d;                            // in [-hist_len, T)
            if (c0 >= len) continue;
            const uint32_t h0 = (pos32 + (uint32_t)c0) & mask;
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
            continue;
        }
        if ((uint32_t)f >= (uint32_t)fa.n_filters) continue;      // a filter outside the table is silent
        const int32_t t0 = min(max(filter_ptr[f], 0), fa.n_taps);
        const int32_t t1 = min(max(filter_ptr[f + 1], t0), fa.n_taps);
        const int32_t K = min(t1 - t0, min(kFirMaxTaps, da.hist_len + 1));
        if (K == 0) continue;
        const int32_t d = min(max(link_delay[k], 0), da.hist_len - (K - 1));
        const int32_t base = tile0 - d - (K - 1);                 // win[i] is column base + i; base >= -hist_len
        if (base >= len) continue;                                // the whole window is silence (block-uniform)
        const int32_t Kp = (K + kFirChunk - 1) & ~(kFirChunk - 1);
        if (staged) __syncthreads();                              // the link before has read win and the taps
        staged = true;
        // kMixTile + Kp <= 2 * kMixTile: a thread stages at most two groups of 8, at win + tid * 8 and, for the first
        // Kp / 8 threads, at win + i1.  Its two sample loads and its three tap loads (g[q] = h[K - 1 - q] inside
        // 0 ... K - 1, else 0; the index clamped into the filter, the value selected) are issued before any is used.
        const int32_t i1 = kMixTile + tid * 8;
        const bool second = i1 < kMixTile + Kp;
        bool whole0, whole1;
        const int16_t* a0 = fir_group_addr(p, ring, base + tid * 8, len, pos32, mask, whole0);
        const int16_t* a1 = fir_group_addr(p, ring, base + i1, len, pos32, mask, whole1);
        store16 w0 = *reinterpret_cast<const store16*>(a0);
        store16 w1 = *reinterpret_cast<const store16*>(a1);
        const int16_t* h = filter_taps + t0;
        const int32_t q = K - 1 - 2 * tid;                        // h's index of g[2 * tid]
        const uint32_t hm = (uint32_t)(uint16_t)h[min(max(q + 1, 0), K - 1)];
        const uint32_t h0 = (uint32_t)(uint16_t)h[min(max(q, 0), K - 1)];
        const uint32_t h1 = (uint32_t)(uint16_t)h[min(max(q - 1, 0), K - 1)];
        const uint32_t gm = (q + 1 >= 0 && q + 1 < K) ? hm : 0u;  // g[2 * tid - 1]
        const uint32_t g0 = q >= 0 ? h0 : 0u;                     // g[2 * tid]
        const uint32_t g1 = q - 1 >= 0 ? h1 : 0u;                 // g[2 * tid + 1]
        if (!whole0) w0 = fir_group_edge(p, ring, base + tid * 8, len, pos32, mask);
        if (second && !whole1) w1 = fir_group_edge(p, ring, base + i1, len, pos32, mask);
        *reinterpret_cast<fir_u32x4*>(win + tid * 8) = fir_u32x4{w0[0], w0[1], w0[2], w0[3]};
        if (second) *reinterpret_cast<fir_u32x4*>(win + i1) = fir_u32x4{w1[0], w1[1], w1[2], w1[3]};
        if (tid < Kp / 2 + 8) {
            tap_even[tid] = g0 | (g1 << 16);
            tap_odd[tid] = gm | (g0 << 16);
        }
        __syncthreads();
        const uint32_t* words = reinterpret_cast<const uint32_t*>(win) + tid * 4;
        int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int32_t c = 0; c < Kp / 2; c += kFirChunk / 2) {     // (c: the chunk's first packed tap word)
            uint32_t S[12], E[8], O[8];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const fir_u32x4 t = *reinterpret_cast<const fir_u32x4*>(words + c + 4 * q);
                S[4 * q] = t[0], S[4 * q + 1] = t[1], S[4 * q + 2] = t[2], S[4 * q + 3] = t[3];
            }
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const fir_u32x4 e = *reinterpret_cast<const fir_u32x4*>(tap_even + c + 4 * q);
                const fir_u32x4 o = *reinterpret_cast<const fir_u32x4*>(tap_odd + c + 4 * q);
                E[4 * q] = e[0], E[4 * q + 1] = e[1], E[4 * q + 2] = e[2], E[4 * q + 3] = e[3];
                O[4 * q] = o[0], O[4 * q + 1] = o[1], O[4 * q + 2] = o[2], O[4 * q + 3] = o[3];
            }
#pragma unroll
            for (int pp = 0; pp < 4; pp++)
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    v[2 * pp] = fir_dot2(S[pp + m], E[m], v[2 * pp]);
                    v[2 * pp + 1] = fir_dot2(S[pp + m], O[m], v[2 * pp + 1]);
                }
        }
        if (K == Kp) {                                            // tap_odd's last word: (g[Kp - 1], 0)
            const fir_u32x4 t = *reinterpret_cast<const fir_u32x4*>(words + Kp / 2);
            const uint32_t o = tap_odd[Kp / 2];
#pragma unroll
            for (int pp = 0; pp < 4; pp++) v[2 * pp + 1] = fir_dot2(t[pp], o, v[2 * pp + 1]);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] += __mul24(g, min(max(v[j] >> 14, -32768), 32767)) >> 15;
    }
    if (!live) return;                                            // behind the last barrier
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

}  // namespace afsk

extern "C" {

int afsk_live_mix_filtered_check(const int32_t* h_row_ptr, const int32_t* h_link_src, const int32_t* h_link_gain_q15,
                                 const int32_t* h_link_delay, const int32_t* h_link_filter, int32_t n_out, int32_t n_src,
                                 int32_t n_links, int32_t hist_len, const int32_t* h_filter_ptr,
                                 const int16_t* h_filter_taps, int32_t n_filters, int32_t n_taps) {
    const std::string me = "afsk_live_mix_filtered_check: ";
    auto bad = [&](const std::string& what) { return afsk::fail(AFSK_E_INVALID_ARG, me + what); };
    if (n_filters < 0 || n_taps < 0) return bad("negative count");
    if (!h_filter_ptr) return bad("null filter_ptr");
    if (n_taps > 0 && !h_filter_taps) return bad("null filter_taps");
    if (n_links > 0 && !h_link_filter) return bad("null link_filter");
    if (int rc = afsk_live_mix_delayed_check(h_row_ptr, h_link_src, h_link_gain_q15, h_link_delay, n_out, n_src,
                                             n_links, hist_len))
        return rc;
    return afsk::no_throw([&] {
        if (h_filter_ptr[0] != 0) return bad("filter_ptr[0] must be 0");
        for (int32_t f = 0; f < n_filters; f++) {
            const int64_t K = (int64_t)h_filter_ptr[f + 1] - h_filter_ptr[f];
            if (h_filter_ptr[f + 1] > n_taps)
                return bad("filter_ptr rises above n_taps = " + std::to_string(n_taps) + " at filter " + std::to_string(f));
            if (K < 1 || K > afsk::kFirMaxTaps)
                return bad("filter " + std::to_string(f) + " has " + std::to_string(K) + " taps, outside 1 ... 256");
            int64_t l1 = 0;
            for (int32_t i = h_filter_ptr[f]; i < h_filter_ptr[f + 1]; i++) l1 += std::abs((int32_t)h_filter_taps[i]);
            if (l1 > afsk::kFirMaxL1)
                return bad("filter " + std::to_string(f) + " has a sum of |taps| of " + std::to_string(l1) +
                           ", above 65535");
        }
        if (h_filter_ptr[n_filters] != n_taps) return bad("filter_ptr must end at n_taps = " + std::to_string(n_taps));
        for (int32_t k = 0; k < n_links; k++) {
            const int32_t f = h_link_filter[k];
            if (f < -1 || f >= n_filters)
                return bad("link " + std::to_string(k) + " names filter " + std::to_string(f) + " outside -1 ... " +
                           std::to_string(n_filters - 1));
            if (f < 0) continue;
            const int64_t reach = (int64_t)h_link_delay[k] + (h_filter_ptr[f + 1] - h_filter_ptr[f]) - 1;
            if (reach > hist_len)
                return bad("link " + std::to_string(k) + " has a reach (delay + taps - 1) of " + std::to_string(reach) +
                           ", above hist_len = " + std::to_string(hist_len));
        }
        return (int)AFSK_OK;
    });
}

int afsk_live_mix_filtered(const int16_t* src, int64_t src_row_stride, int32_t n_src, const int32_t* d_src_lens_or_null,
                           const int32_t* d_row_ptr, const int32_t* d_link_src, const int32_t* d_link_gain_q15,
                           const int32_t* d_link_delay, const int32_t* d_link_filter, int32_t n_links, int16_t* out,
                           int64_t out_row_stride, int32_t n_out, int32_t n_samples,
                           const int32_t* d_noise_scale_q24_or_null, uint32_t noise_seed, uint32_t noise_idx_base,
                           int64_t* d_pos, int16_t* d_history, int32_t hist_len, const int32_t* d_filter_ptr,
                           const int16_t* d_filter_taps, int32_t n_filters, int32_t n_taps, void* hip_stream) {
    const char* const me = "afsk_live_mix_filtered: ";
    auto bad = [&](const char* what) { return afsk::fail(AFSK_E_INVALID_ARG, std::string(me) + what); };
    if (n_src < 0 || n_links < 0 || n_out < 0 || n_filters < 0 || n_taps < 0) return bad("negative count");
    if (n_samples < 0 || n_samples > afsk::kMixMaxSamples) return bad("n_samples must lie in 0 ... 2^20");
    if (!afsk::mix_hist_len_valid(hist_len)) return bad("hist_len must be a power of two in 8 ... 2^20");
    if ((n_src > 0 && (!src || !d_history)) || (n_out > 0 && (!out || !d_row_ptr)) ||
        (n_links > 0 && (!d_link_src || !d_link_gain_q15 || !d_link_delay || !d_link_filter)) || !d_pos ||
        !d_filter_ptr || (n_taps > 0 && !d_filter_taps))
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
    afsk::MixFirArgs a{};
    a.d.m.out = out;
    a.d.m.out_stride = n_out > 1 ? out_row_stride : 0;
    a.d.m.src_stride = n_src > 1 ? src_row_stride : 0;
    a.d.m.n_src = n_src;
    a.d.m.n_links = n_links;
    a.d.m.n_samples = n_samples;
    a.d.m.tiles = (n_samples + afsk::kMixTile - 1) / afsk::kMixTile;
    a.d.m.noise_seed = noise_seed;
    a.d.m.noise_idx_base = noise_idx_base;
    a.d.hist_len = hist_len;
    a.n_filters = n_filters;
    a.n_taps = n_taps;
    afsk::MixDelayArgs h = a.d;                                   // the history kernel's: its own columns and tiles
    h.first = n_samples > hist_len ? n_samples - hist_len : 0;
    h.m.tiles = (n_samples - h.first + afsk::kMixTile - 1) / afsk::kMixTile;
    const int64_t blocks = (int64_t)a.d.m.tiles * n_out, hblocks = (int64_t)h.m.tiles * n_src;
    if (blocks > 0x7fffffffll) return bad("n_out * tiles exceeds 2^31 - 1");
    if (hblocks > 0x7fffffffll) return bad("n_src * tiles of the history exceeds 2^31 - 1");
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_mix_fir_kernel, dim3((uint32_t)blocks), dim3(afsk::kMixThreads), 0, st, a, src,
                       d_src_lens_or_null, d_row_ptr, d_link_src, d_link_gain_q15, d_link_delay, d_link_filter,
                       d_filter_ptr, d_filter_taps, (const int16_t*)d_history, d_noise_scale_q24_or_null,
                       (const int64_t*)d_pos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_fir_kernel");
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
