// afsk_live_mix.hip -- the live medium (afsk_live_mix, afsk_live_mix_check, include/afsk_amd.h): the air between live
// stations.  Every output row is the clipped sum of the source rows its links name, each scaled by a Q15 gain, with
// optional receiver noise that continues from call to call.
//
// A call is one launch, or two in order on the caller's stream when a position is kept:
//   live_mix_kernel          one block per (output row, tile of kMixTile columns), one thread per 8 consecutive columns.
//                            The row's link range, and every link's source, gain and length, are the same in all
//                            lanes: they are scalar loads and the link loop is a scalar loop.  A link whose 8 columns lie
//                            inside its source's length is one 16-byte load at a 2-byte-aligned address (store16's
//                            alignment, the default cache policy: a source row is read by every row that hears it) and
//                            8 x (24-bit multiply, shift, add); one that straddles the length reads the columns below it
//                            one by one, and one at or past it reads nothing.  The sums are clipped, a row with a noise
//                            scale draws afsk_add_noise_batch's noise on top, and the 8 columns leave as one 16-byte
//                            store (one by one in the tile that holds column T).
//   live_mix_advance_kernel  one thread: *pos += T, behind the mix that read it.
// Nothing is read through a table entry before it was clamped: the row's link range to [0, n_links] and 32768 links,
// a source index to [0, n_src) (else the link is silent), a length to [0, T], a gain to +-65535.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end): it uses that
// file's store16, noise_key and noise_term, and afsk_live_tx.hip's includes.
#include <string>

namespace afsk {

constexpr int kMixThreads = 256;
constexpr int kMixTile = kMixThreads * 8;                       // columns per block
constexpr int32_t kMixMaxSamples = 1 << 20;
constexpr int32_t kMixMaxDegree = 32768;                        // links per row: 32768 * 65535 < 2^31
constexpr int32_t kMixMaxGain = 65535;                          // |gain|: 65535 * 32768 < 2^31

struct MixArgs {
    int16_t* out;
    int64_t out_stride;
    int64_t src_stride;
    int32_t n_src;
    int32_t n_links;
    int32_t n_samples;
    int32_t tiles;                  // blocks per output row
    uint32_t noise_seed;
    uint32_t noise_idx_base;
};

// (the block order: xcd_block -- an XCD takes 8 consecutive (row, tile) blocks, so rows that are neighbours, and the
// neighbouring source rows they read, meet in one L2.  Against the plain order, -DAFSK_LIVE_MIX_PLAIN_ORDER, it measured
// x 0.975 at T = 2048 and x 0.997 at T = 8192 on three unity sources per row: DESIGN.md 8.17)
__global__ __launch_bounds__(kMixThreads) void live_mix_kernel(MixArgs a, const int16_t* __restrict__ src,
                                                               const int32_t* __restrict__ src_lens,
                                                               const int32_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ link_src,
                                                               const int32_t* __restrict__ link_gain,
                                                               const int32_t* __restrict__ noise_scale,
                                                               const int64_t* __restrict__ pos_ptr) {
#ifdef AFSK_LIVE_MIX_PLAIN_ORDER
    const int32_t bid = (int32_t)blockIdx.x;
#else
    const int32_t bid = xcd_block((int)blockIdx.x, (int)gridDim.x);
#endif
    const int32_t r = bid / a.tiles;
    const int32_t tile = bid - r * a.tiles;
    const int32_t T = a.n_samples;
    const int32_t j0 = tile * kMixTile + (int32_t)threadIdx.x * 8;
    if (j0 >= T) return;
    const int32_t lo = min(max(row_ptr[r], 0), a.n_links);
    const int32_t hi = min(max(row_ptr[r + 1], lo), lo + min(a.n_links - lo, kMixMaxDegree));
    int32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t k = lo; k < hi; k++) {
        const int32_t s = link_src[k];
        const int32_t g = min(max(link_gain[k], -kMixMaxGain), kMixMaxGain);
        int32_t len = 0;                                          // a source outside the matrix is silent
        if ((uint32_t)s < (uint32_t)a.n_src) len = src_lens ? min(max(src_lens[s], 0), T) : T;
        if (j0 >= len) continue;
        const int16_t* p = src + (int64_t)s * a.src_stride + j0;
        if (j0 + 8 <= len) {
            const store16 w = *reinterpret_cast<const store16*>(p);
#pragma unroll
            for (int d = 0; d < 4; d++) {
                acc[2 * d] += __mul24(g, (int32_t)(int16_t)(w[d] & 0xffffu)) >> 15;
                acc[2 * d + 1] += __mul24(g, (int32_t)w[d] >> 16) >> 15;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j0 + j < len) acc[j] += __mul24(g, (int32_t)p[j]) >> 15;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = min(max(acc[j], -32768), 32767);
    const int32_t scale = noise_scale ? noise_scale[r] : 0;
    if (scale != 0) {                                             // per row: block-uniform
        const uint32_t key = noise_key(a.noise_seed, a.noise_idx_base + (uint32_t)r);
        const uint32_t t0 = (uint32_t)(pos_ptr ? (uint64_t)*pos_ptr : 0ull) + (uint32_t)j0;
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

__global__ void live_mix_advance_kernel(int64_t* pos, int32_t n_samples) { *pos += n_samples; }

}  // namespace afsk

extern "C" {

int afsk_live_mix_check(const int32_t* h_row_ptr, const int32_t* h_link_src, const int32_t* h_link_gain_q15,
                        int32_t n_out, int32_t n_src, int32_t n_links) {
    if (n_out < 0 || n_src < 0 || n_links < 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: negative count");
    if (!h_row_ptr) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: null row_ptr");
    if (n_links > 0 && (!h_link_src || !h_link_gain_q15))
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: null link_src or link_gain_q15");
    return afsk::no_throw([&] {
        if (h_row_ptr[0] != 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: row_ptr[0] must be 0");
        for (int32_t r = 0; r < n_out; r++) {
            if (h_row_ptr[r + 1] < h_row_ptr[r])
                return afsk::fail(AFSK_E_INVALID_ARG,
                                  "afsk_live_mix_check: row_ptr falls at output row " + std::to_string(r));
            if ((int64_t)h_row_ptr[r + 1] - h_row_ptr[r] > afsk::kMixMaxDegree)
                return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: output row " + std::to_string(r) +
                                                          " has more than 32768 links");
        }
        if (h_row_ptr[n_out] != n_links)
            return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: row_ptr must end at n_links");
        for (int32_t k = 0; k < n_links; k++) {
            if (h_link_src[k] < 0 || h_link_src[k] >= n_src)
                return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: link " + std::to_string(k) + " names source " +
                                                          std::to_string(h_link_src[k]) + " outside 0 ... n_src - 1");
            if (h_link_gain_q15[k] < -afsk::kMixMaxGain || h_link_gain_q15[k] > afsk::kMixMaxGain)
                return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix_check: link " + std::to_string(k) +
                                                          " has a gain outside -65535 ... 65535");
        }
        return (int)AFSK_OK;
    });
}

int afsk_live_mix(const int16_t* src, int64_t src_row_stride, int32_t n_src, const int32_t* d_src_lens_or_null,
                  const int32_t* d_row_ptr, const int32_t* d_link_src, const int32_t* d_link_gain_q15, int32_t n_links,
                  int16_t* out, int64_t out_row_stride, int32_t n_out, int32_t n_samples,
                  const int32_t* d_noise_scale_q24_or_null, uint32_t noise_seed, uint32_t noise_idx_base,
                  int64_t* d_pos_or_null, void* hip_stream) {
    if (n_src < 0 || n_links < 0 || n_out < 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: negative count");
    if (n_samples < 0 || n_samples > afsk::kMixMaxSamples)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: n_samples must lie in 0 ... 2^20");
    if ((n_src > 0 && !src) || (n_out > 0 && (!out || !d_row_ptr)) || (n_links > 0 && (!d_link_src || !d_link_gain_q15)))
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: null pointer argument");
    if ((n_src > 1 && src_row_stride < n_samples) || (n_out > 1 && out_row_stride < n_samples))
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: a row stride below n_samples (rows would overlap)");
    if (n_src > 0 && n_out > 0 && n_samples > 0) {
        // the bytes the kernel may touch: columns [0, n_samples) of every row (at most 2^31 rows of 2^62 bytes apart)
        const uintptr_t s0 = (uintptr_t)src, o0 = (uintptr_t)out;
        const uintptr_t s1 = s0 + 2 * ((uintptr_t)(n_src - 1) * (uintptr_t)(n_src > 1 ? src_row_stride : 0) + n_samples);
        const uintptr_t o1 = o0 + 2 * ((uintptr_t)(n_out - 1) * (uintptr_t)(n_out > 1 ? out_row_stride : 0) + n_samples);
        if (s0 < o1 && o0 < s1) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: out overlaps src");
    }
    if (n_samples == 0 || n_out == 0) return AFSK_OK;
    afsk::MixArgs a{};
    a.out = out;
    a.out_stride = n_out > 1 ? out_row_stride : 0;
    a.src_stride = n_src > 1 ? src_row_stride : 0;
    a.n_src = n_src;
    a.n_links = n_links;
    a.n_samples = n_samples;
    a.tiles = (n_samples + afsk::kMixTile - 1) / afsk::kMixTile;
    a.noise_seed = noise_seed;
    a.noise_idx_base = noise_idx_base;
    const int64_t blocks = (int64_t)a.tiles * n_out;
    if (blocks > 0x7fffffffll) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_mix: n_out * tiles exceeds 2^31 - 1");
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_mix_kernel, dim3((uint32_t)blocks), dim3(afsk::kMixThreads), 0, st, a, src,
                       d_src_lens_or_null, d_row_ptr, d_link_src, d_link_gain_q15, d_noise_scale_q24_or_null,
                       (const int64_t*)d_pos_or_null);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_kernel");
    if (d_pos_or_null) {
        hipLaunchKernelGGL(afsk::live_mix_advance_kernel, dim3(1), dim3(1), 0, st, d_pos_or_null, n_samples);
        e = hipGetLastError();
        if (e != hipSuccess) return afsk::hip_fail(e, "launch live_mix_advance_kernel");
    }
    return AFSK_OK;
}

}  // extern "C"
