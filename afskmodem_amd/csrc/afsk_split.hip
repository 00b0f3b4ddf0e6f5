// afsk_split.hip -- sequence-parallel demodulation: one stream split over many wavefronts
// (afsk_split_plan_* / afsk_demod_batch_split, include/afsk_amd.h).
//
// Every other demod kernel gives one stream to one wave for its whole length, which fills the card only from
// ~2048 streams on (one wave alone moves 8-9 GB/s).  A batch of few, long streams -- one long recording, a large
// payload, the live gate's bursts -- needs the work of ONE stream spread over many waves.  The reference's
// __decodeBits (afskmodem.py:354-381) splits cleanly once the clock index is known:
//   * clock recovery (ref:322-339) reads only the first 4096 samples;
//   * symbol k sits at sample ci + k * bf; its decision (ref:342-351) and its squelch flag
//     (getAmplitude(chunk) >= amp_end, ref:375) depend on that symbol's samples alone;
//   * only the terminator scan (ref:361-366, 386-390) and the squelch stop (ref:372-376) are sequential, and
//     both are "first position where a bit pattern holds" over the per-symbol bits;
//   * ECC.decode (ref:154-163) and __bitsToBytes (ref:393-399) are independent per codeword / byte.
// So three launches, in order on the caller's stream (a captured graph of them is a linear chain):
//   A  split_clock_kernel    one wave per stream: the product's clock recovery on the first 8 KiB (the same
//                            helpers as the single-pass kernels), ci into scratch; refusals (TOO_SHORT, BAD_LENGTH)
//                            get their outputs here.
//   B  split_segment_*       one wave per SEGMENT: a fixed run of seg_symbols symbols (a multiple of 64, so a wave
//                            owns whole 64-bit bitmap words and needs no atomics) of one stream.  It writes two
//                            bitmaps -- decisions and "loud" flags -- and, with soft outputs, the margins.
//                            bit_frames 40 (1200 baud): LDS-DMA passes of 64 symbols through a four-slot ring;
//                            every other rate: direct range-checked loads (correct, not tuned).
//   C  split_finish_kernel   one wave per stream: terminator and squelch stop by ballots over the bitmap words,
//                            then the Hamming decode + byte pack with one lane per output byte.
// Every output field equals what afsk_demod_batch_ex writes for the same input (bit-exact by construction; the
// GPU suite checks it against the reference fixture and the oracle).
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end): build.sh has a
// fixed list of translation units, and everything included here from the demod headers is inline or a template.
#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "../../include/afsk_amd.h"
#include "afsk_capi_internal.h"
#include "afsk_demod_impl.h"

namespace afsk {

constexpr int kSplitDefaultSymbols = 1024;          // 16 bitmap words, 80 KiB of samples at 1200 baud
constexpr int kSplitSlots = 4;                      // pass buffers per wave (3 passes in flight)
constexpr int kSplitPassBytes = 5120;               // 64 symbols of 40 samples
constexpr int kSplitSlotBytes = kSplitPassBytes + 16;   // + the 16 bytes the last lane's shifted read reaches into
constexpr int kSplitRequests = 6;                   // LDS-DMA requests per pass: 5 x 1 KiB + one 16-byte tail

struct SplitArgs {
    const int16_t* samples;
    const int64_t* stream_offset;
    const int32_t* stream_len;
    // plan (device)
    const int32_t* bit_frames;
    const int32_t* plan_len;
    const int64_t* word_off;           // first bitmap word of stream s
    const int32_t* seg_stream;
    const int32_t* seg_k0;
    int32_t seg_begin;                 // the segments [seg_begin, seg_end) of this stage-B launch
    int32_t seg_end;
    int32_t seg_symbols;
    int32_t n_streams;
    int32_t amp_end;
    // scratch
    int32_t* ci;                       // [n] clock index, -1 = refused (outputs written by stage A)
    unsigned long long* dec;           // decision words; bit j of word w = symbol 64 w + j
    unsigned long long* loud;          // squelch flags, same layout
    // outputs
    uint8_t* out_bytes;
    int32_t out_stride;
    int32_t* out_nbytes;
    int32_t* out_nbits;
    int32_t* out_clock_idx;
    int32_t* out_term_frame;
    int32_t* out_status;
    int32_t* out_corrected;
    int32_t* out_margins;
    int32_t margin_stride;
};

__device__ __forceinline__ uint32_t split_amp_thr(int32_t amp_end, int bf) {   // as the single-pass kernels
    return (uint32_t)(amp_end < 0 ? 0 : (amp_end > 40000 ? 40000 : amp_end)) * (uint32_t)bf;
}

// ------------------------------------------------------------------------------------------- stage A
__global__ __launch_bounds__(64) void split_clock_kernel(SplitArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kFastWaveLdsProduct];
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x;
    if (s >= a.n_streams) return;
    const int32_t len = a.stream_len[s];
    int32_t status = -1;
    // the range rule of afsk_demod_batch, and a device length beyond the one the plan was sized for
    if ((uint32_t)len > (uint32_t)kMaxStreamLen || len > a.plan_len[s]) status = AFSK_ST_BAD_LENGTH;
    else if (len < kSync) status = AFSK_ST_TOO_SHORT;           // ref:323-325
    if (status >= 0) {
        if (lane == 0) {
            a.out_nbytes[s] = 0; a.out_nbits[s] = 0; a.out_clock_idx[s] = -1;
            a.out_term_frame[s] = -1; a.out_status[s] = status;
            if (a.out_corrected) a.out_corrected[s] = 0;
            a.ci[s] = -1;
        }
        return;
    }
    const int bf = a.bit_frames[s];
    FastRing fr;
    fr.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(a.samples + a.stream_offset[s]), 0, len * 2, 0x00020000);
    fr.ring = lds;
    fr.lane = lane;
    fr.template issue_run<0, 8>(0);                              // samples 0 .. 4095: the sync window
    fr.next = 8;
    int ci;
    if (bf == 40) {
        if (clock_index_is_zero<40, 8>(fr)) ci = 0;              // ref:332-337 (no search needed)
        else ci = recover_clock_index_lanes<40, false, 8>(fr);
    } else {
        wait_vmcnt<0>();
        ci = recover_clock_index_rt(fr, bf);
    }
    wait_vmcnt<0>();                                             // no DMA may land after the wave has left
    if (lane == 0) a.ci[s] = ci;
}

// ------------------------------------------------------------------------------------------- stage B
// The segment's symbols [k0, kend) of one stream, whose clock index is known.  Returns false when there is nothing to do.
struct SegmentView {
    const int16_t* xs;
    int32_t len, ci, k0, kend, K;
    unsigned long long* dec;
    unsigned long long* loud;
    int32_t* margins;
    int32_t mlim;
};

__device__ __forceinline__ bool split_segment(const SplitArgs& a, int g, int bf, SegmentView& v) {
    const int s = a.seg_stream[g];
    const int32_t ci = a.ci[s];
    if (ci < 0) return false;                                    // refused by stage A
    v.len = a.stream_len[s];
    v.ci = ci;
    v.K = (v.len - ci - 1) / bf;                                 // symbols with i < len - bf (ref:362, 372)
    v.k0 = a.seg_k0[g];
    v.kend = v.K < v.k0 + a.seg_symbols ? v.K : v.k0 + a.seg_symbols;
    if (v.kend <= v.k0) return false;                            // past the stream's last symbol
    v.xs = a.samples + a.stream_offset[s];
    v.dec = a.dec + a.word_off[s] + (v.k0 >> 6);
    v.loud = a.loud + a.word_off[s] + (v.k0 >> 6);
    v.margins = a.out_margins ? a.out_margins + (int64_t)s * a.margin_stride : nullptr;
    v.mlim = v.K < a.margin_stride ? v.K : a.margin_stride;
    return true;
}

// bit_frames 40: pass p (symbols k0 + 64 p ...) lives in slot p % 4, requested from the 16-byte-aligned stream byte
// G + 5120 p below the symbol's first byte, so symbol j of a pass starts at slot byte e + 80 j with e = (2 q0) & 15,
// the same for every pass of the segment.  A lane reads its 80 bytes as six aligned ds_read_b128 and drops A = e / 4
// dwords (ODD: and one more sample, v_alignbyte) in registers: eight compile-time forms instead of unaligned reads.
template <int A, bool ODD>
__device__ __forceinline__ void split_passes_40(const SplitArgs& a, const SegmentView& v, uint8_t* lds, int lane) {
    constexpr int BF = 40, Q = BF / 4;
    constexpr uint32_t FULL = 65535u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)v.xs, 0, v.len * 2, 0x00020000);
    const int np = (v.kend - v.k0 + 63) >> 6;
    const int G = (2 * (v.ci + v.k0 * BF)) & ~15;
    const uint32_t amp_thr = split_amp_thr(a.amp_end, BF);
    auto issue = [&](int p) {
        uint8_t* slot = lds + (p & (kSplitSlots - 1)) * kSplitSlotBytes;
        const int src = G + p * kSplitPassBytes;
#pragma unroll
        for (int r = 0; r < 5; r++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, AFSK_LDS(slot + r * 1024), 16, lane * 16, src + r * 1024, 0, 0);
        if (lane == 0)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, AFSK_LDS(slot + kSplitPassBytes), 16, 0, src + kSplitPassBytes, 0, 0);
    };
    const int pre = np < kSplitSlots ? np : kSplitSlots;
    for (int p = 0; p < pre; p++) issue(p);
    for (int p = 0; p < np; p++) {
        // passes p + 1 .. min(np - 1, p + 3) may still be in flight
        const int younger = (np - 1 - p) < (kSplitSlots - 1) ? (np - 1 - p) : (kSplitSlots - 1);
        switch (younger) {
            case 0: wait_vmcnt<0>(); break;
            case 1: wait_vmcnt<kSplitRequests>(); break;
            case 2: wait_vmcnt<2 * kSplitRequests>(); break;
            default: wait_vmcnt<3 * kSplitRequests>(); break;
        }
        const uint8_t* src = lds + (p & (kSplitSlots - 1)) * kSplitSlotBytes + lane * 80;
        constexpr int NW = A + 20 + (ODD ? 1 : 0);               // dwords the lane needs
        uint32_t W[24];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (4 * i < NW) {
                const u32x4 t = *reinterpret_cast<const u32x4*>(src + 16 * i);
                W[4 * i] = t[0]; W[4 * i + 1] = t[1]; W[4 * i + 2] = t[2]; W[4 * i + 3] = t[3];
            } else {
                W[4 * i] = W[4 * i + 1] = W[4 * i + 2] = W[4 * i + 3] = 0;
            }
        }
        uint32_t x[20];
#pragma unroll
        for (int d = 0; d < 20; d++) x[d] = ODD ? __builtin_amdgcn_alignbyte(W[A + d + 1], W[A + d], 2) : W[A + d];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the slot has been read: it may be refilled
        if (p + kSplitSlots < np) issue(p + kSplitSlots);
        // ref:342-351 as afsk_demod_rounds_fast.h: mark = hi,lo,hi,lo quarters (ref:80-85), space = hi,hi,lo,lo (ref:68-77)
        const uint32_t h0 = hi_sad<0, 5>(x), h1 = hi_sad<5, 10>(x), h2 = hi_sad<10, 15>(x), h3 = hi_sad<15, 20>(x);
        const uint32_t mark = 2u * FULL * Q + h0 + h2 - h1 - h3;
        const uint32_t space = 2u * FULL * Q + h0 + h1 - h2 - h3;
        const uint32_t md = mark / (uint32_t)BF, sd = space / (uint32_t)BF;
        const int32_t k = v.k0 + 64 * p + lane;
        if (v.margins && k < v.mlim) v.margins[k] = (int32_t)sd - (int32_t)md;
        const uint64_t bits = __ballot(md < sd);                 // ref:348-351
        const uint64_t loud = __ballot(loud_enough(quiet_sum<0, 20>(x), (uint32_t)BF, amp_thr));   // ref:375
        if (lane == 0) { v.dec[p] = bits; v.loud[p] = loud; }
    }
}

__global__ __launch_bounds__(64) void split_segment_40_kernel(SplitArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSplitSlots * kSplitSlotBytes];
    const int lane = threadIdx.x & 63;
    const int g = a.seg_begin + (int)blockIdx.x;
    if (g >= a.seg_end) return;
    SegmentView v;
    if (!split_segment(a, g, 40, v)) return;
    const int e = (2 * (v.ci + v.k0 * 40)) & 15;
    switch (e) {
        case 0: split_passes_40<0, false>(a, v, lds, lane); break;
        case 2: split_passes_40<0, true>(a, v, lds, lane); break;
        case 4: split_passes_40<1, false>(a, v, lds, lane); break;
        case 6: split_passes_40<1, true>(a, v, lds, lane); break;
        case 8: split_passes_40<2, false>(a, v, lds, lane); break;
        case 10: split_passes_40<2, true>(a, v, lds, lane); break;
        case 12: split_passes_40<3, false>(a, v, lds, lane); break;
        default: split_passes_40<3, true>(a, v, lds, lane); break;
    }
}

// Every other rate: one lane per symbol, its samples by range-checked 2-byte buffer loads, quarter by quarter.
__global__ __launch_bounds__(256) void split_segment_rt_kernel(SplitArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = a.seg_begin + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= a.seg_end) return;
    const int bf = a.bit_frames[a.seg_stream[g]];
    SegmentView v;
    if (!split_segment(a, g, bf, v)) return;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)v.xs, 0, v.len * 2, 0x00020000);
    const int q = bf >> 2;
    const uint32_t amp_thr = split_amp_thr(a.amp_end, bf);
    const int np = (v.kend - v.k0 + 63) >> 6;
    for (int p = 0; p < np; p++) {
        const int32_t k = v.k0 + 64 * p + lane;
        const bool valid = k < v.kend;
        const int base = 2 * (v.ci + (valid ? k : v.k0) * bf);  // (idle lanes re-read the segment's first symbol)
        uint32_t h[4];
        uint32_t amp = 0;
        for (int qi = 0; qi < 4; qi++) {
            uint32_t hq = 0;
            for (int j = 0; j < q; j++) {
                const int32_t x = (int16_t)__builtin_amdgcn_raw_buffer_load_b16(rsrc, base + 2 * (qi * q + j), 0, 0);
                const uint32_t lim = x > 512 ? 65535u : (x < -512 ? 0u : 32768u);   // ref:287-296, biased
                hq += 65535u - lim;                                                 // SAD against 32767
                amp += (uint32_t)(x < 0 ? -x : x);                                  // ref:94-98
            }
            h[qi] = hq;
        }
        const uint32_t full = 65535u * (uint32_t)q;
        const uint32_t mark = 2u * full + h[0] + h[2] - h[1] - h[3];
        const uint32_t space = 2u * full + h[0] + h[1] - h[2] - h[3];
        const uint32_t md = mark / (uint32_t)bf, sd = space / (uint32_t)bf;
        if (v.margins && valid && k < v.mlim) v.margins[k] = (int32_t)sd - (int32_t)md;
        const uint64_t bits = __ballot(valid && md < sd);
        const uint64_t loud = __ballot(valid && amp >= amp_thr);
        if (lane == 0) { v.dec[p] = bits; v.loud[p] = loud; }
    }
}

// ------------------------------------------------------------------------------------------- stage C
__device__ __forceinline__ uint64_t split_valid_bits(int64_t w, int64_t nw, int32_t K) {
    return (w == nw - 1 && (K & 63)) ? ((1ull << (K & 63)) - 1ull) : ~0ull;
}

__global__ __launch_bounds__(256) void split_finish_kernel(SplitArgs a) {
    const int lane = threadIdx.x & 63;
    const int s = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (s >= a.n_streams) return;
    const int32_t ci = a.ci[s];
    if (ci < 0) return;                                          // refused: stage A wrote the outputs
    const int32_t len = a.stream_len[s];
    const int bf = a.bit_frames[s];
    const int32_t K = (len - ci - 1) / bf;
    const int32_t nw = (K + 63) >> 6;
    const unsigned long long* dec = a.dec + a.word_off[s];
    const unsigned long long* loud = a.loud + a.word_off[s];
    // terminator: first k with decisions (k-3 .. k) = 1,0,0,0 (ref:361-366, 386-390; the window starts as 0,0,0,0)
    int32_t term = -1;
    for (int32_t w0 = 0; w0 < nw; w0 += 64) {
        const int32_t w = w0 + lane;
        uint32_t cand = 0xFFFFFFFFu;
        if (w < nw) {
            const uint64_t d = dec[w] & split_valid_bits(w, nw, K);
            const uint64_t pv = w > 0 ? dec[w - 1] : 0ull;
            const uint64_t b3 = (d << 3) | (pv >> 61), b2 = (d << 2) | (pv >> 62), b1 = (d << 1) | (pv >> 63);
            const uint64_t hit = b3 & ~b2 & ~b1 & ~d & split_valid_bits(w, nw, K);
            if (hit) cand = (uint32_t)w * 64u + (uint32_t)__builtin_ctzll(hit);
        }
        const uint32_t m = wave_min_u32(cand);
        if (m != 0xFFFFFFFFu) { term = (int32_t)m; break; }
    }
    int32_t first = K, nbits = 0;                                // no terminator: term_frame after the last symbol
    if (term >= 0) {
        first = term + 1;                                        // first data symbol (ref:368)
        // squelch stop: first quiet symbol from `first` on (ref:372-376), else the end of the stream
        int32_t stop = K;
        for (int32_t w0 = first >> 6; w0 < nw; w0 += 64) {
            const int32_t w = w0 + lane;
            uint32_t cand = 0xFFFFFFFFu;
            if (w < nw) {
                uint64_t qt = ~loud[w] & split_valid_bits(w, nw, K);
                if (w == (first >> 6)) qt &= ~0ull << (first & 63);
                if (qt) cand = (uint32_t)w * 64u + (uint32_t)__builtin_ctzll(qt);
            }
            const uint32_t m = wave_min_u32(cand);
            if (m != 0xFFFFFFFFu) { stop = (int32_t)m; break; }
        }
        nbits = stop - first;
    }
    // ECC.decode (ref:154-163) + __bitsToBytes (ref:393-399): byte b = codewords 2b, 2b + 1 = data bits 14b ... 14b + 13
    const int32_t n_cw = nbits / 7;
    const int32_t nbytes = n_cw >> 1;
    uint8_t* row = a.out_bytes + (int64_t)s * a.out_stride;
    int32_t corrected = 0;
    for (int32_t b = lane; b < (n_cw + 1) >> 1; b += 64) {
        const int32_t P = first + 14 * b;
        const int32_t w = P >> 6, sh = P & 63;
        uint64_t v = dec[w] >> sh;
        if (sh > 50 && w + 1 < nw) v |= dec[w + 1] << (64 - sh);
        const uint32_t cw0 = (uint32_t)v & 0x7Fu, cw1 = (uint32_t)(v >> 7) & 0x7Fu;
        corrected += hamming_syndrome(cw0) != 0u;
        if (2 * b + 1 < n_cw) {
            corrected += hamming_syndrome(cw1) != 0u;
            if (b < a.out_stride) row[b] = (uint8_t)((hamming_nibble(cw0) << 4) | hamming_nibble(cw1));
        }
    }
    corrected = __builtin_amdgcn_readlane(wave_incl_scan_dpp(corrected), 63);
    if (lane == 0) {
        a.out_nbytes[s] = nbytes;
        a.out_nbits[s] = nbits;
        a.out_clock_idx[s] = ci;
        a.out_term_frame[s] = ci + first * bf;                   // ref:368
        a.out_status[s] = nbits == 0 ? AFSK_ST_NO_DATA : AFSK_ST_OK;   // ref:422-424
        if (a.out_corrected) a.out_corrected[s] = corrected;
    }
}

// ------------------------------------------------------------------------------------------- host side
// Host-side layout of a plan: segments and bitmap words per stream from the lengths the plan is built for
// (ceil(len / bf) symbols: the clock index is not known yet).  Scratch = [n] int32 clock indices (rounded up to
// 256 bytes) + two bitmaps of total_words 64-bit words each.
struct SplitLayout {
    int32_t seg_symbols = 0;
    int64_t n_segments = 0;
    int64_t total_words = 0;
    int64_t ci_bytes = 0;
    int64_t scratch_bytes = 0;
};

static int split_layout(const int32_t* len, const int32_t* bf, int32_t n, int32_t segment_symbols, SplitLayout& L,
                        std::vector<int64_t>* word_off, std::vector<int32_t>* seg_stream, std::vector<int32_t>* seg_k0) {
    if (n < 0 || segment_symbols < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n > 0 && (!len || !bf)) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (segment_symbols % 64) return fail(AFSK_E_INVALID_ARG, "segment_symbols must be a multiple of 64 (0 = default)");
    L.seg_symbols = segment_symbols ? segment_symbols : kSplitDefaultSymbols;
    for (int32_t s = 0; s < n; s++) {
        if (!bf_valid(bf[s])) return fail_bit_frames();
        if (len[s] < 0 || len[s] > AFSK_MAX_STREAM_LEN)
            return fail(AFSK_E_INVALID_ARG, "stream_len outside 0 ... AFSK_MAX_STREAM_LEN");
    }
    // segments of the 1200-baud streams first (their own stage-B kernel), then the rest, each in stream order
    if (word_off) word_off->assign((size_t)n, 0);
    for (int pass = 0; pass < 2; pass++) {
        for (int32_t s = 0; s < n; s++) {
            if ((bf[s] == 40) != (pass == 0)) continue;
            const int64_t nsym = len[s] < AFSK_SYNC_WINDOW ? 0 : (len[s] + (int64_t)bf[s] - 1) / bf[s];
            const int64_t nseg = (nsym + L.seg_symbols - 1) / L.seg_symbols;
            if (seg_stream)
                for (int64_t k = 0; k < nseg; k++) { seg_stream->push_back(s); seg_k0->push_back((int32_t)(k * L.seg_symbols)); }
            L.n_segments += nseg;
        }
    }
    for (int32_t s = 0; s < n; s++) {
        const int64_t nsym = len[s] < AFSK_SYNC_WINDOW ? 0 : (len[s] + (int64_t)bf[s] - 1) / bf[s];
        if (word_off) (*word_off)[(size_t)s] = L.total_words;
        L.total_words += (nsym + 63) / 64;
    }
    if (L.n_segments > std::numeric_limits<int32_t>::max())
        return fail(AFSK_E_INVALID_ARG, "more than 2^31 - 1 segments: use a larger segment_symbols");
    L.ci_bytes = ((4 * (int64_t)n + 255) / 256) * 256;
    L.scratch_bytes = L.ci_bytes + 16 * L.total_words;
    return AFSK_OK;
}

}  // namespace afsk

struct afsk_split_plan {
    afsk::DeviceState state;           // bit_frames [n] | plan_len [n] | word_off [n] (8-aligned) | seg_stream | seg_k0
    int32_t n = 0;
    afsk::SplitLayout L;
    int32_t n_seg40 = 0;               // segments [0, n_seg40) are 1200-baud ones
    int32_t *bf = nullptr, *plen = nullptr, *seg_stream = nullptr, *seg_k0 = nullptr;
    int64_t* word_off = nullptr;
};

extern "C" {

int afsk_split_scratch_bytes(const int32_t* stream_len_host, const int32_t* bit_frames_host, int32_t n_streams,
                             int32_t segment_symbols, int64_t* out_scratch_bytes, int32_t* out_n_segments) {
    afsk::SplitLayout L;
    if (int rc = afsk::split_layout(stream_len_host, bit_frames_host, n_streams, segment_symbols, L, nullptr, nullptr,
                                    nullptr))
        return rc;
    if (out_scratch_bytes) *out_scratch_bytes = L.scratch_bytes;
    if (out_n_segments) *out_n_segments = (int32_t)L.n_segments;
    return AFSK_OK;
}

int afsk_split_plan_create(const int32_t* stream_len_host, const int32_t* bit_frames_host, int32_t n_streams,
                           int32_t segment_symbols, afsk_split_plan** out_plan) {
    if (!out_plan) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out_plan = nullptr;
    return afsk::no_throw([&] {
        std::vector<int64_t> word_off;
        std::vector<int32_t> seg_stream, seg_k0;
        std::unique_ptr<afsk_split_plan> pl(new afsk_split_plan());
        if (int rc = afsk::split_layout(stream_len_host, bit_frames_host, n_streams, segment_symbols, pl->L, &word_off,
                                        &seg_stream, &seg_k0))
            return rc;
        pl->n = n_streams;
        int32_t n40 = 0;
        for (size_t g = 0; g < seg_stream.size(); g++) n40 += bit_frames_host[seg_stream[g]] == 40;
        pl->n_seg40 = n40;
        const size_t n = (size_t)n_streams, ns = seg_stream.size();
        const size_t o_plen = 4 * n, o_woff = ((8 * n + 7) / 8) * 8, o_seg = o_woff + 8 * n, o_k0 = o_seg + 4 * ns;
        const size_t bytes = o_k0 + 4 * ns;
        std::vector<uint8_t> h(bytes);
        if (n) {
            std::memcpy(h.data(), bit_frames_host, 4 * n);
            std::memcpy(h.data() + o_plen, stream_len_host, 4 * n);
            std::memcpy(h.data() + o_woff, word_off.data(), 8 * n);
        }
        if (ns) {
            std::memcpy(h.data() + o_seg, seg_stream.data(), 4 * ns);
            std::memcpy(h.data() + o_k0, seg_k0.data(), 4 * ns);
        }
        if (int rc = pl->state.create("afsk_split_plan_create", (int64_t)bytes, 0, h.data(), 0, (int64_t)bytes))
            return rc;
        uint8_t* d = pl->state.ptr();       // (null without streams: every offset is 0)
        pl->bf = reinterpret_cast<int32_t*>(d);
        pl->plen = reinterpret_cast<int32_t*>(d + o_plen);
        pl->word_off = reinterpret_cast<int64_t*>(d + o_woff);
        pl->seg_stream = reinterpret_cast<int32_t*>(d + o_seg);
        pl->seg_k0 = reinterpret_cast<int32_t*>(d + o_k0);
        *out_plan = pl.release();
        return AFSK_OK;
    });
}

int afsk_split_plan_info(const afsk_split_plan* plan, int32_t* out_n_streams, int32_t* out_n_segments,
                         int64_t* out_scratch_bytes) {
    if (!plan) return afsk::fail(AFSK_E_INVALID_ARG, "null plan");
    if (out_n_streams) *out_n_streams = plan->n;
    if (out_n_segments) *out_n_segments = (int32_t)plan->L.n_segments;
    if (out_scratch_bytes) *out_scratch_bytes = plan->L.scratch_bytes;
    return AFSK_OK;
}

int afsk_split_plan_destroy(afsk_split_plan* plan) {
    delete plan;      // the segment table; the caller has synchronised its launches
    return AFSK_OK;
}

int afsk_demod_batch_split(const afsk_split_plan* plan, const int16_t* samples, const int64_t* stream_offset,
                           const int32_t* stream_len, int32_t amp_end_threshold, void* d_scratch,
                           uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                           int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status,
                           int32_t* out_corrected, int32_t* out_margins, int32_t margin_stride, void* hip_stream) {
    const afsk::DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                               out_corrected, out_margins, margin_stride};
    if (!plan) return afsk::fail(AFSK_E_INVALID_ARG, "null plan");
    if (o.negative()) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (plan->n == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || o.missing() || !d_scratch)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = plan->state.check_current()) return rc;
    afsk::SplitArgs a = o.args<afsk::SplitArgs>(samples, stream_offset, stream_len, amp_end_threshold, plan->n);
    a.bit_frames = plan->bf; a.plan_len = plan->plen; a.word_off = plan->word_off;
    a.seg_stream = plan->seg_stream; a.seg_k0 = plan->seg_k0;
    a.seg_symbols = plan->L.seg_symbols;
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    a.ci = reinterpret_cast<int32_t*>(scratch);
    a.dec = reinterpret_cast<unsigned long long*>(scratch + plan->L.ci_bytes);
    a.loud = a.dec + plan->L.total_words;
    const hipStream_t st = (hipStream_t)hip_stream;
    // A, B (1200 baud), B (every other rate), C: strictly in order on the caller's stream
    hipLaunchKernelGGL(afsk::split_clock_kernel, dim3(plan->n), dim3(64), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch split_clock_kernel");
    const int32_t nseg = (int32_t)plan->L.n_segments;
    if (plan->n_seg40 > 0) {
        a.seg_begin = 0; a.seg_end = plan->n_seg40;
        hipLaunchKernelGGL(afsk::split_segment_40_kernel, dim3(plan->n_seg40), dim3(64), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return afsk::hip_fail(e, "launch split_segment_40_kernel");
    }
    if (nseg > plan->n_seg40) {
        a.seg_begin = plan->n_seg40; a.seg_end = nseg;
        hipLaunchKernelGGL(afsk::split_segment_rt_kernel, dim3((nseg - plan->n_seg40 + 3) / 4), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return afsk::hip_fail(e, "launch split_segment_rt_kernel");
    }
    hipLaunchKernelGGL(afsk::split_finish_kernel, dim3((plan->n + 3) / 4), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return afsk::hip_fail(e, "launch split_finish_kernel");
    return AFSK_OK;
}

}  // extern "C"
