// afsk_live_fade.hip -- the faded live medium (afsk_live_mix_faded, afsk_live_mix_faded_check, include/afsk_amd.h):
// afsk_live_mix_filtered with a gain that moves along a cyclic Q15 track per link.  A link with track f (L knots, a
// power of two; 2^p samples per knot) and offset o has, at medium time t = pos + j, the envelope
//   u = (uint32)(pos + j) + o;   n = (u >> p) & (L - 1);   m = (n + 1) & (L - 1);   q = u & (2^p - 1)
//   e = knot[n] + (((int32)(knot[m] - knot[n]) * q) >> p)
// and contributes (g * clamp16((e * x) >> 15)) >> 15, x being what the link contributes in the filtered medium before
// its gain: the delayed sample, or the filter's clamped output.  e lies between its two knots, so inside 0 ... 65535,
// and both products fit int32 (65535 * 32768 < 2^31).
//
// A call is three launches, in order on the caller's stream:
//   live_mix_fade_kernel     live_mix_fir_kernel's superset: its block and thread shape, its block order, its scalar link
//                            loop, its clip, noise and store.  A link without a track (-1) takes that kernel's code: the
//                            unfiltered three-way path or the staged dot2 path.  A link with one has the same two paths
//                            with the envelope between the sample and the gain: the unfiltered one takes its 8 samples
//                            as one 16-byte load or through fir_group_edge (the three-way decision, the samples kept
//                            apart instead of added), the filtered one multiplies v[8] as it was staged.  The envelope
//                            of a thread's 8 columns needs at most three consecutive knots (p >= 3: the 8 columns
//                            cross at most one knot boundary), n0, n0 + 1 and n0 + 2 of u0 = pos + j0 + o.  Every lane
//                            loads its three as uint16 through the vector cache: the track, shift and offset are the
//                            same in all lanes, a wave's 512 columns touch at most 66 consecutive knots (132 bytes:
//                            two or three cache lines shared by all its lanes), and the unfiltered path keeps running
//                            without a barrier, which staging the knots in LDS would put into it.  Per column the
//                            knot pair is chosen by the low bit of (u >> p) against n0's: 2^(32 - p) is even, so the
//                            choice also holds where u wraps past 2^32.  61 VGPRs, the fir kernel's LDS, no scratch;
//                            held to 8 waves per SIMD (see at the kernel).
//   live_mix_history_kernel  afsk_live_delay.hip's, unchanged.
//   live_mix_advance_kernel  afsk_live_mix.hip's.
// Nothing is read through a table entry before it was clamped: what live_mix_fir_kernel clamps; a fade index outside
// -1 ... n_fades - 1 is silent; fade_ptr entries to [0, n_knots] and the second not below the first; L is the largest
// power of two at or below min(the entries' difference, 65536), no knots are silent; the shift to 3 ... 15.  Knots and
// offsets are values, not addresses.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end), behind
// afsk_live_fir.hip, whose MixFirArgs, fir_group_addr, fir_group_edge and fir_dot2 it uses.

namespace afsk {

constexpr int32_t kFadeMaxKnots = 65536;                        // knots of one track
constexpr int32_t kFadeMinShift = 3, kFadeMaxShift = 15;        // log2 of the samples per knot

struct MixFadeArgs {
    MixFirArgs f;
    int32_t n_fades;
    int32_t n_knots;                // entries of fade_knots
};

// One link's track as the lanes use it, clamped: kn its first knot, lmask = L - 1, p its shift, off the link's offset.
struct FadeTrack {
    const uint16_t* kn;
    uint32_t lmask;
    uint32_t p;
    uint32_t off;
};

// The envelope of the 8 columns whose first has u = u0.
__device__ __forceinline__ void fade_env8(int32_t (&e)[8], const FadeTrack& tr, uint32_t u0) {
    const uint32_t n0 = u0 >> tr.p;
    const int32_t k0 = (int32_t)tr.kn[n0 & tr.lmask];
    const int32_t k1 = (int32_t)tr.kn[(n0 + 1u) & tr.lmask];
    const int32_t k2 = (int32_t)tr.kn[(n0 + 2u) & tr.lmask];
    const uint32_t qmask = (1u << tr.p) - 1u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t u = u0 + (uint32_t)j;
        const bool next = (((u >> tr.p) ^ n0) & 1u) != 0u;
        const int32_t a = next ? k1 : k0, b = next ? k2 : k1;
        e[j] = a + (__mul24(b - a, (int32_t)(u & qmask)) >> tr.p);
    }
}

__device__ __forceinline__ int32_t fade_term(int32_t g, int32_t e, int32_t x) {
    return __mul24(g, min(max(__mul24(e, x) >> 15, -32768), 32767)) >> 15;
}

// 8 waves per SIMD, as the kernels it extends: left alone the compiler keeps 101 scalar registers (17 pointer arguments
// and the argument structs) over the link loop, which leaves room for 7 waves, and this kernel's time follows the waves
// it has in flight (measured: x 1.12 of live_mix_fir_kernel on the same unfaded links at 7 waves, x 1.04 at 8).  Held
// to 8 it parks 17 scalars in VGPR lanes (v_writelane / v_readlane, no scratch).
__global__ __launch_bounds__(kMixThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
void live_mix_fade_kernel(MixFadeArgs ga, const int16_t* __restrict__ src,
                          const int32_t* __restrict__ src_lens,
                          const int32_t* __restrict__ row_ptr,
                          const int32_t* __restrict__ link_src,
                          const int32_t* __restrict__ link_gain,
                          const int32_t* __restrict__ link_delay,
                          const int32_t* __restrict__ link_filter,
                          const int32_t* __restrict__ link_fade,
                          const uint32_t* __restrict__ link_fade_offset,
                          const int32_t* __restrict__ filter_ptr,
                          const int16_t* __restrict__ filter_taps,
                          const int32_t* __restrict__ fade_ptr,
                          const int32_t* __restrict__ fade_shift,
                          const uint16_t* __restrict__ fade_knots,
                          const int16_t* __restrict__ history,
                          const int32_t* __restrict__ noise_scale,
                          const int64_t* __restrict__ pos_ptr) {
    __shared__ __attribute__((aligned(16))) int16_t win[kFirWin];
    __shared__ __attribute__((aligned(16))) uint32_t tap_even[kFirTapWords];
    __shared__ __attribute__((aligned(16))) uint32_t tap_odd[kFirTapWords];
    const MixFirArgs& fa = ga.f;
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
        const int32_t fd = link_fade[k];
        const bool faded = fd != -1;
        FadeTrack tr{fade_knots, 0u, (uint32_t)kFadeMinShift, 0u};
        if (faded) {
            if ((uint32_t)fd >= (uint32_t)ga.n_fades) continue;   // a track outside the table is silent
            const int32_t q0 = min(max(fade_ptr[fd], 0), ga.n_knots);
            const int32_t q1 = min(max(fade_ptr[fd + 1], q0), ga.n_knots);
            const int32_t n = min(q1 - q0, kFadeMaxKnots);
            if (n == 0) continue;                                 // no knots: silent
            tr.kn = fade_knots + q0;
            tr.lmask = (1u << (31 - __clz(n))) - 1u;              // L: n rounded down to a power of two
            tr.p = (uint32_t)min(max(fade_shift[fd], kFadeMinShift), kFadeMaxShift);
            tr.off = link_fade_offset[k];
        }
        const uint32_t u0 = pos32 + (uint32_t)j0 + tr.off;
        const int32_t f = link_filter[k];
        if (f == -1) {                                            // live_mix_delay_kernel's link
            if (!live) continue;
            const int32_t d = min(max(link_delay[k], 0), da.hist_len);
            const int32_t c0 = j0 - d;                            // in [-hist_len, T)
            if (c0 >= len) continue;
            const uint32_t h0 = (pos32 + (uint32_t)c0) & mask;
            if (faded) {                                          // the same three ways, the samples kept apart
                bool whole;
                const int16_t* a0 = fir_group_addr(p, ring, c0, len, pos32, mask, whole);
                store16 w = *reinterpret_cast<const store16*>(a0);
                int32_t e[8];
                fade_env8(e, tr, u0);
                if (!whole) w = fir_group_edge(p, ring, c0, len, pos32, mask);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    acc[2 * q] += fade_term(g, e[2 * q], (int32_t)(int16_t)(w[q] & 0xffffu));
                    acc[2 * q + 1] += fade_term(g, e[2 * q + 1], (int32_t)w[q] >> 16);
                }
                continue;
            }
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
        // staged as live_mix_fir_kernel stages (see there)
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
        if (faded) {
            int32_t e[8];
            fade_env8(e, tr, u0);
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += fade_term(g, e[j], min(max(v[j] >> 14, -32768), 32767));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] += __mul24(g, min(max(v[j] >> 14, -32768), 32767)) >> 15;
        }
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

int afsk_live_mix_faded_check(const int32_t* h_row_ptr, const int32_t* h_link_src, const int32_t* h_link_gain_q15,
                              const int32_t* h_link_delay, const int32_t* h_link_filter, const int32_t* h_link_fade,
                              int32_t n_out, int32_t n_src, int32_t n_links, int32_t hist_len,
                              const int32_t* h_filter_ptr, const int16_t* h_filter_taps, int32_t n_filters,
                              int32_t n_taps, const int32_t* h_fade_ptr, const int32_t* h_fade_shift, int32_t n_fades,
                              int32_t n_knots) {
    const std::string me = "afsk_live_mix_faded_check: ";
    auto bad = [&](const std::string& what) { return afsk::fail(AFSK_E_INVALID_ARG, me + what); };
    if (n_fades < 0 || n_knots < 0) return bad("negative count");
    if (!h_fade_ptr) return bad("null fade_ptr");
    if (n_fades > 0 && !h_fade_shift) return bad("null fade_shift");
    if (n_links > 0 && !h_link_fade) return bad("null link_fade");
    if (int rc = afsk_live_mix_filtered_check(h_row_ptr, h_link_src, h_link_gain_q15, h_link_delay, h_link_filter, n_out,
                                              n_src, n_links, hist_len, h_filter_ptr, h_filter_taps, n_filters, n_taps))
        return rc;
    return afsk::no_throw([&] {
        if (h_fade_ptr[0] != 0) return bad("fade_ptr[0] must be 0");
        for (int32_t f = 0; f < n_fades; f++) {
            const int64_t L = (int64_t)h_fade_ptr[f + 1] - h_fade_ptr[f];
            if (h_fade_ptr[f + 1] > n_knots)
                return bad("fade_ptr rises above n_knots = " + std::to_string(n_knots) + " at track " + std::to_string(f));
            if (L < 1 || L > afsk::kFadeMaxKnots || (L & (L - 1)) != 0)
                return bad("track " + std::to_string(f) + " has " + std::to_string(L) +
                           " knots, not a power of two in 1 ... 65536");
            if (h_fade_shift[f] < afsk::kFadeMinShift || h_fade_shift[f] > afsk::kFadeMaxShift)
                return bad("track " + std::to_string(f) + " has a shift of " + std::to_string(h_fade_shift[f]) +
                           ", outside 3 ... 15");
        }
        if (h_fade_ptr[n_fades] != n_knots) return bad("fade_ptr must end at n_knots = " + std::to_string(n_knots));
        for (int32_t k = 0; k < n_links; k++) {
            const int32_t f = h_link_fade[k];
            if (f < -1 || f >= n_fades)
                return bad("link " + std::to_string(k) + " names track " + std::to_string(f) + " outside -1 ... " +
                           std::to_string(n_fades - 1));
        }
        return (int)AFSK_OK;
    });
}

int afsk_live_mix_faded(const int16_t* src, int64_t src_row_stride, int32_t n_src, const int32_t* d_src_lens_or_null,
                        const int32_t* d_row_ptr, const int32_t* d_link_src, const int32_t* d_link_gain_q15,
                        const int32_t* d_link_delay, const int32_t* d_link_filter, int32_t n_links, int16_t* out,
                        int64_t out_row_stride, int32_t n_out, int32_t n_samples,
                        const int32_t* d_noise_scale_q24_or_null, uint32_t noise_seed, uint32_t noise_idx_base,
                        int64_t* d_pos, int16_t* d_history, int32_t hist_len, const int32_t* d_filter_ptr,
                        const int16_t* d_filter_taps, int32_t n_filters, int32_t n_taps, const int32_t* d_link_fade,
                        const uint32_t* d_link_fade_offset, const int32_t* d_fade_ptr, const int32_t* d_fade_shift,
                        const uint16_t* d_fade_knots, int32_t n_fades, int32_t n_knots, void* hip_stream) {
    const char* const me = "afsk_live_mix_faded: ";
    auto bad = [&](const char* what) { return afsk::fail(AFSK_E_INVALID_ARG, std::string(me) + what); };
    if (n_src < 0 || n_links < 0 || n_out < 0 || n_filters < 0 || n_taps < 0 || n_fades < 0 || n_knots < 0)
        return bad("negative count");
    if (n_samples < 0 || n_samples > afsk::kMixMaxSamples) return bad("n_samples must lie in 0 ... 2^20");
    if (!afsk::mix_hist_len_valid(hist_len)) return bad("hist_len must be a power of two in 8 ... 2^20");
    if ((n_src > 0 && (!src || !d_history)) || (n_out > 0 && (!out || !d_row_ptr)) ||
        (n_links > 0 && (!d_link_src || !d_link_gain_q15 || !d_link_delay || !d_link_filter || !d_link_fade ||
                         !d_link_fade_offset)) ||
        !d_pos || !d_filter_ptr || (n_taps > 0 && !d_filter_taps) || !d_fade_ptr || (n_fades > 0 && !d_fade_shift) ||
        (n_knots > 0 && !d_fade_knots))
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
    afsk::MixFadeArgs a{};
    afsk::MixArgs& m = a.f.d.m;
    m.out = out;
    m.out_stride = n_out > 1 ? out_row_stride : 0;
    m.src_stride = n_src > 1 ? src_row_stride : 0;
    m.n_src = n_src;
    m.n_links = n_links;
    m.n_samples = n_samples;
    m.tiles = (n_samples + afsk::kMixTile - 1) / afsk::kMixTile;
    m.noise_seed = noise_seed;
    m.noise_idx_base = noise_idx_base;
    a.f.d.hist_len = hist_len;
    a.f.n_filters = n_filters;
    a.f.n_taps = n_taps;
    a.n_fades = n_fades;
    a.n_knots = n_knots;
    afsk::MixDelayArgs h = a.f.d;                                 // the history kernel's: its own columns and tiles
    h.first = n_samples > hist_len ? n_samples - hist_len : 0;
    h.m.tiles = (n_samples - h.first + afsk::kMixTile - 1) / afsk::kMixTile;
    const int64_t blocks = (int64_t)m.tiles * n_out, hblocks = (int64_t)h.m.tiles * n_src;
    if (blocks > 0x7fffffffll) return bad("n_out * tiles exceeds 2^31 - 1");
    if (hblocks > 0x7fffffffll) return bad("n_src * tiles of the history exceeds 2^31 - 1");
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_mix_fade_kernel, dim3((uint32_t)blocks), dim3(afsk::kMixThreads), 0, st, a, src,
                       d_src_lens_or_null, d_row_ptr, d_link_src, d_link_gain_q15, d_link_delay, d_link_filter,
                       d_link_fade, d_link_fade_offset, d_filter_ptr, d_filter_taps, d_fade_ptr, d_fade_shift,
                       d_fade_knots, (const int16_t*)d_history, d_noise_scale_q24_or_null, (const int64_t*)d_pos);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_fade_kernel");
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
