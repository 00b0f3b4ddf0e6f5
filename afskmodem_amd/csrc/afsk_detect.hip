// afsk_detect.hip -- the rate detector (afsk_detect_rate_batch, include/afsk_amd.h): which of up to 36 candidate
// bit_frames values a stream was sent at, decided on the device from the stream's first 4096 samples, so that the answer
// feeds afsk_demod_batch's per-stream bit_frames without a host hop.
//
// Per candidate bf, with tc = the training cycle of that rate (mark ++ space, 2 bf samples, ref:88-91) and x = the raw
// samples (all integer, exact):
//   total(i) = sum_{j < 2bf} |tc[j] - x[i + j]|          i in [0, 4096 - 2bf)     (the sums of ref:327-331)
//   d(i)     = total(i) / (2bf),   ci = the first i with minimal d(i)             (the clock index of ref:332-337)
//   n        = (4096 - 2bf - 1 - ci) / (2bf) + 1                                  (whole cycles from ci on)
//   score    = (sum_{k < n} total(ci + k 2bf)) / (n 2bf)                          (0 ... 65535)
// The stream's rate is the candidate of smallest score, the earliest of the list on a tie.
//
// detect_rate_kernel: one workgroup of 256 threads per stream.
//   1. the 8 KB window with two 16-byte loads per thread (a thread holds 16 consecutive samples), an exclusive int32
//      prefix sum E[0 .. 4096) of it in LDS (16 KB; |E| < 2^27)
//   2. a template sample is 32767 or -32768 and |32767 - x| = 32767 - x, |-32768 - x| = x + 32768 for every int16 x, so
//      total(i) = 65535 bf + E[i] - 2 E[i+q] + 2 E[i+2q] - 2 E[i+3q] + 2 E[i+bf] - 2 E[i+bf+h] + E[i+2bf]   (q = bf/4,
//      h = bf/2): seven LDS reads, the lanes of a wave at consecutive i -- consecutive banks, conflict-free
//   3. the four waves take the candidates in turn (wave w: w, w + 4, ...); a lane keeps the minimum of (d << 12) | i over
//      its offsets (d < 2^16, i < 2^12: one unsigned min is the first-minimum argmin), a wave reduction gives ci; the
//      lanes then take the n <= 511 cycle starts, a wave sum gives the score
//   4. wave 0 takes min (score << 6) | position over the candidates -- the tie rule -- and the minimum without the winner
// The division by 2bf is a multiplication: total < 2^28 and the divisor W = 2bf <= 4088 is wave-uniform, so with
// t = max(0, ceil(log2 W) - 4) and m = ceil(2^(32+t) / W) (m < 2^32 because 2^t < W; computed on the host and passed by
// value) mulhi(total, m) >> t is exact: m W - 2^(32+t) < W and total W < 2^(32+t).
// No scratch, no atomics; every global write is an ordinary vector store by wave 0.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end).
#include "afsk_capi_internal.h"

namespace afsk {

constexpr int kDetectWindow = AFSK_SYNC_WINDOW;             // samples read per stream
constexpr int kDetectMaxCand = AFSK_DETECT_MAX_CANDIDATES;
constexpr int kDetectThreads = 256;
static_assert(kDetectWindow == 16 * kDetectThreads, "a thread holds 16 samples of the window");
static_assert(kDetectMaxCand <= 64, "the candidates' scores are reduced by one wave, their position takes 6 bits");

struct DetectArgs {
    const int16_t* samples;
    const int64_t* stream_offset;
    const int32_t* stream_len;
    int32_t* out_bit_frames;
    int32_t* out_score;
    int32_t* out_runner_up;
    int32_t* out_clock_idx;
    int32_t* out_scores;                  // [n_streams, n_cand] or null
    int32_t n_streams;
    int32_t n_cand;
    int32_t cand[kDetectMaxCand];         // the candidate list, by value: no upload, nothing to keep alive
    uint32_t magic[kDetectMaxCand];       // ceil(2^(32 + shift) / (2 cand))
    uint8_t shift[kDetectMaxCand];
};

// (m, t) of the exact division by W described above
inline void detect_divisor(int32_t W, uint32_t& m, uint8_t& t) {
    int lg = 0;
    while ((1 << lg) < W) lg++;
    t = (uint8_t)(lg > 4 ? lg - 4 : 0);
    m = (uint32_t)((((uint64_t)1 << (32 + t)) + (uint64_t)W - 1) / (uint64_t)W);
}

__device__ __forceinline__ uint32_t detect_wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ int detect_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// total(i) - 65535 bf from the prefix sums
__device__ __forceinline__ int detect_total(const int* E, int i, int q, int bf) {
    const int a = E[i] + E[i + 2 * bf];
    const int b = E[i + 2 * q] - E[i + q] + E[i + bf] - E[i + 3 * q] - E[i + bf + 2 * q];
    return a + 2 * b;
}

__global__ __launch_bounds__(kDetectThreads) void detect_rate_kernel(DetectArgs a) {
    __shared__ int E[kDetectWindow];
    __shared__ int wave_total[4];
    __shared__ int c_score[64], c_ci[64], c_bf[64];                   // (a slot per lane of the wave that reduces them)
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t len = a.stream_len[s];
    // a stream shorter than the window, or of a length outside 0 ... AFSK_MAX_STREAM_LEN: nothing of it is read
    if (len < kDetectWindow || len > kMaxStreamLen) {
        if (tid == 0) {
            a.out_bit_frames[s] = 0;
            a.out_score[s] = -1;
            a.out_runner_up[s] = -1;
            a.out_clock_idx[s] = -1;
        }
        if (a.out_scores && tid < a.n_cand) a.out_scores[(int64_t)s * a.n_cand + tid] = -1;
        return;
    }
    // 1. the window and its exclusive prefix sum
    const int16_t* src = a.samples + a.stream_offset[s] + 16 * tid;
    const vec16 v0 = *reinterpret_cast<const vec16*>(src);
    const vec16 v1 = *reinterpret_cast<const vec16*>(src + 8);
    int x[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        x[2 * k] = (int16_t)(v0[k] & 0xffffu);
        x[2 * k + 1] = (int32_t)v0[k] >> 16;
        x[8 + 2 * k] = (int16_t)(v1[k] & 0xffffu);
        x[8 + 2 * k + 1] = (int32_t)v1[k] >> 16;
    }
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) mine += x[k];
    int incl = mine;                                      // inclusive scan over the wave's lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int w = 0; w < wave; w++) run += wave_total[w];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        E[16 * tid + k] = run;
        run += x[k];
    }
    __syncthreads();
    // 2., 3. the candidates, wave by wave
    for (int c = wave; c < a.n_cand; c += 4) {
        const int bf = a.cand[c];
        const uint32_t m = a.magic[c];
        const int t = a.shift[c];
        const int q = bf >> 2, W = 2 * bf;
        const int base = 65535 * bf;
        const int n_off = kDetectWindow - W;
        uint32_t best = 0xffffffffu;
        for (int i = lane; i < n_off; i += 64) {
            const uint32_t total = (uint32_t)(base + detect_total(E, i, q, bf));
            const uint32_t d = __umulhi(total, m) >> t;
            best = min(best, (d << 12) | (uint32_t)i);
        }
        const int ci = __builtin_amdgcn_readfirstlane((int)(detect_wave_min(best) & 4095u));
        const int n = (n_off - 1 - ci) / W + 1;
        int sum = 0;
        for (int k = lane; k < n; k += 64) sum += base + detect_total(E, ci + k * W, q, bf);
        sum = detect_wave_sum(sum);
        if (lane == 0) {
            c_score[c] = (int)((uint32_t)sum / (uint32_t)(n * W));
            c_ci[c] = ci;
            c_bf[c] = bf;
        }
    }
    __syncthreads();
    // 4. the smallest score, the earliest candidate on a tie; the smallest of the others
    if (wave == 0) {
        const bool in = lane < a.n_cand;
        const uint32_t key = in ? ((uint32_t)c_score[lane] << 6) | (uint32_t)lane : 0xffffffffu;
        const int win = (int)(detect_wave_min(key) & 63u);
        const uint32_t other = detect_wave_min(in && lane != win ? (uint32_t)c_score[lane] : 0xffffffffu);
        if (lane == 0) {
            a.out_bit_frames[s] = c_bf[win];
            a.out_score[s] = c_score[win];
            a.out_runner_up[s] = (int32_t)other;          // (0xffffffff = -1 with one candidate)
            a.out_clock_idx[s] = c_ci[win];
        }
        if (a.out_scores && in) a.out_scores[(int64_t)s * a.n_cand + lane] = c_score[lane];
    }
}

}  // namespace afsk

extern "C" {

int afsk_detect_rate_batch(const int16_t* samples, const int64_t* stream_offset, const int32_t* stream_len,
                           int32_t n_streams, const int32_t* cand_bit_frames_host, int32_t n_cand,
                           int32_t* out_bit_frames, int32_t* out_score, int32_t* out_runner_up, int32_t* out_clock_idx,
                           int32_t* out_scores, void* hip_stream) {
    using namespace afsk;
    if (n_streams < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_cand < 1 || n_cand > kDetectMaxCand)
        return fail(AFSK_E_INVALID_ARG, "n_cand must be 1 ... AFSK_DETECT_MAX_CANDIDATES");
    if (!cand_bit_frames_host) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    DetectArgs a{};
    for (int k = 0; k < n_cand; k++) {
        if (!bf_valid(cand_bit_frames_host[k])) return fail_bit_frames();
        a.cand[k] = cand_bit_frames_host[k];
        detect_divisor(2 * a.cand[k], a.magic[k], a.shift[k]);
    }
    if (n_streams == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || !out_bit_frames || !out_score || !out_runner_up || !out_clock_idx)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    a.samples = samples; a.stream_offset = stream_offset; a.stream_len = stream_len;
    a.out_bit_frames = out_bit_frames; a.out_score = out_score; a.out_runner_up = out_runner_up;
    a.out_clock_idx = out_clock_idx; a.out_scores = out_scores;
    a.n_streams = n_streams; a.n_cand = n_cand;
    hipLaunchKernelGGL(detect_rate_kernel, dim3((uint32_t)n_streams), dim3(kDetectThreads), 0, (hipStream_t)hip_stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch detect_rate_kernel");
}

}  // extern "C"
