// afsk_live_level.hip -- the live receivers' level tracker (afsk_live_create_stream_leveled / afsk_live_level /
// afsk_live_level_reset / afsk_live_level_check, include/afsk_amd.h): a noise floor F and a decaying peak P per channel,
// followed block by block on the device, and the gate / squelch pair of the channel derived from them ahead of every
// push.  A leveled receiver is a streaming receiver (afsk_live_stream.hip; fixed rate, tapped or auto) whose threshold
// pair lives in the per-channel arrays even when all pairs agree; its push is the PER_CHANNEL cell it always was, which
// reads thr_start[c] / thr_end[c] once per push, and the streaming sink takes its per-symbol squelch from the same
// amp_end.  live_level_kernel runs in front of that push on the same stream and rewrites the two entries, so no existing
// kernel changes.
//
// The rule (integer, exact).  For channel c the tracker walks the whole 2048-sample blocks the push will
// walk -- cl = pos & 2047 carried samples, len = the channel's sample count, nblk = (cl + len) / 2048, block 0 of a push
// with a carry = carry[0, cl) + chunk[0, 2048 - cl) -- and takes every block's amplitude A exactly as the gate does
// (live_load_chunk_block / live_load_carry_block, block_abs_sum >> 11).  A block with any column inside the channel's
// clamped mute range is skipped: not loaded, no update.  rec = (the channel's gate is recording when the push starts),
// pp = P before the first block; per block
//     P  = A > P ? A : P - ((P - A + (1 << decay_shift) - 1) >> decay_shift)
//     pp = max(pp, P)
//     if (!rec)  F = F < 0 ? A : (A < F ? F - ((F - A + 3) >> 2) : F + ((A - F) >> rise_shift))
// After the walk F and P are stored; unless rec, with Fz = max(F, 0),
//     start = min(65535, max((start_q15 * pp) >> 15, (floor_start_q8 * Fz) >> 8, min_start))
//     end   = min(65535, max((end_q15   * pp) >> 15, (floor_end_q8   * Fz) >> 8, min_end))
// go to thr_start[c] / thr_end[c] and to the channel's state row.  While a burst records the pair stays what it was
// when the burst opened: one pair gates, squelches and demodulates a burst from its first block to its last.
//
// Shape: the gate walk's own -- one wave per channel, four waves per 256-thread block, the next block's four 16-byte
// loads per lane in flight while the current block is summed.  The channel number goes through readfirstlane, so the
// channel's state, length, mute range and level row are scalar loads and everything behind the wave-wide sum (the rule,
// the pair) runs in scalar registers; lane 0 stores.  No LDS, no scratch.  Nothing at or beyond column len of a row is
// read.
//
// AFSK_LIVE_LEVEL_NT (default 1): the chunk loads are nontemporal like the push's (live_load_chunk_block); 0 builds the
// cacheable form (build.sh -DAFSK_LIVE_LEVEL_NT=0).  The push reads the same columns right behind the tracker;
// profiles/live_level_bench.txt has both forms measured on tracker + push together.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), behind
// afsk_live_push.hip.

#ifndef AFSK_LIVE_LEVEL_NT
#define AFSK_LIVE_LEVEL_NT 1
#endif

namespace afsk {

struct LiveLevelArgs {
    const LiveChan* chan;
    const int16_t* carry;
    const int16_t* chunk;
    int64_t chunk_stride;
    const int32_t* chunk_lens;      // int32 [n] or null
    const int32_t* mute;            // int32 [n, 2] or null
    int32_t* state;                 // int32 [n, 4]: floor, peak, start, end
    int32_t* thr_start;             // the receiver's own pair arrays, int32 [n] each
    int32_t* thr_end;
    int32_t chunk_len;
    int32_t n;
    afsk_live_level_params p;
};

__device__ __forceinline__ void live_level_load_block(vec16 (&v)[4], const int16_t* p, int lane) {
#if AFSK_LIVE_LEVEL_NT
    live_load_chunk_block(v, p, lane);
#else
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = *reinterpret_cast<const vec16*>(p + 512 * j + 8 * lane);
#endif
}

__global__ __launch_bounds__(256) void live_level_kernel(LiveLevelArgs a) {
    const int lane = threadIdx.x & 63;
    const int c_lane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c_lane >= a.n) return;
    const int c = __builtin_amdgcn_readfirstlane(c_lane);          // wave-uniform: scalar loads, scalar rule
    const int64_t pos = a.chan[c].pos;
    const bool rec = a.chan[c].mode == 2;
    int32_t len = a.chunk_len;
    if (a.chunk_lens) {
        const int32_t l = a.chunk_lens[c];
        len = l < 0 ? 0 : (l > a.chunk_len ? a.chunk_len : l);
    }
    int32_t mute_lo = 0, mute_hi = 0;                               // the push's clamp (live_gate_walk)
    if (a.mute) {
        const int32_t lo = a.mute[2 * (int64_t)c], hi = a.mute[2 * (int64_t)c + 1];
        mute_lo = lo < 0 ? 0 : (lo > len ? len : lo);
        mute_hi = hi < mute_lo ? mute_lo : (hi > len ? len : hi);
    }
    int32_t* row = a.state + 4 * (int64_t)c;
    int32_t F = row[0], P = row[1];
    int32_t pp = P;
    const int16_t* carry = a.carry + (int64_t)c * kListenBlock;
    const int16_t* src = a.chunk + (int64_t)c * a.chunk_stride;

    const int cl = (int)(pos & (kListenBlock - 1));                 // carried samples
    const int32_t nblk = (int32_t)(((int64_t)cl + len) / kListenBlock);
    // block b has a column inside the muted range (block 0 of a push with a carry starts below column 0)
    auto skip = [&](int32_t b) -> bool {
        const int32_t col0 = b * kListenBlock - cl;
        return mute_lo < mute_hi && mute_lo < col0 + kListenBlock && mute_hi > col0;
    };
    const int32_t round_up = (1 << a.p.decay_shift) - 1;
    vec16 cur[4], nxt[4];
    live_zero_block(cur);
    live_zero_block(nxt);
    if (nblk > 0 && !skip(0)) {
        if (cl > 0) live_load_carry_block(cur, carry, src, cl, lane);
        else live_level_load_block(cur, src, lane);
    }
    for (int32_t b = 0; b < nblk; b++) {
        if (b + 1 < nblk && !skip(b + 1))                           // next block in flight
            live_level_load_block(nxt, src + (int64_t)(b + 1) * kListenBlock - cl, lane);
        if (!skip(b)) {
            const int32_t A = (int32_t)((uint32_t)__builtin_amdgcn_readlane(block_abs_sum(cur), 63) >> 11);
            P = A > P ? A : P - ((P - A + round_up) >> a.p.decay_shift);
            pp = pp > P ? pp : P;
            if (!rec) F = F < 0 ? A : (A < F ? F - ((F - A + 3) >> 2) : F + ((A - F) >> a.p.rise_shift));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) cur[j] = nxt[j];
    }

    const int32_t Fz = F < 0 ? 0 : F;
    auto pair = [&](int32_t q15, int32_t q8, int32_t least) -> int32_t {
        int32_t t = (q15 * pp) >> 15;                               // (65535 * 32768 < 2^31)
        const int32_t f = (q8 * Fz) >> 8;
        t = t > f ? t : f;
        t = t > least ? t : least;
        return t < 65535 ? t : 65535;
    };
    const int32_t start = pair(a.p.start_q15, a.p.floor_start_q8, a.p.min_start);
    const int32_t end = pair(a.p.end_q15, a.p.floor_end_q8, a.p.min_end);
    if (lane == 0) {
        row[0] = F;
        row[1] = P;
        if (!rec) {
            row[2] = start;
            row[3] = end;
            a.thr_start[c] = start;
            a.thr_end[c] = end;
        }
    }
}

// rows of masked channels back to (-1, 0, start0, end0), and their entries of the receiver's pair arrays
__global__ __launch_bounds__(256) void live_level_reset_kernel(int32_t* state, int32_t* thr_start, int32_t* thr_end,
                                                               const uint8_t* mask, int32_t n, int32_t start0,
                                                               int32_t end0) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n && (!mask || mask[c])) {
        int32_t* row = state + 4 * (int64_t)c;
        row[0] = -1;
        row[1] = 0;
        row[2] = start0;
        row[3] = end0;
        thr_start[c] = start0;
        thr_end[c] = end0;
    }
}

inline int live_level_check(const afsk_live_level_params& p) {
    auto ordered = [](int32_t lo, int32_t hi) { return 0 <= lo && lo <= hi && hi <= 65535; };
    if (!ordered(p.end_q15, p.start_q15))
        return fail(AFSK_E_INVALID_ARG, "level: 0 <= end_q15 <= start_q15 <= 65535 must hold");
    if (!ordered(p.floor_end_q8, p.floor_start_q8))
        return fail(AFSK_E_INVALID_ARG, "level: 0 <= floor_end_q8 <= floor_start_q8 <= 65535 must hold");
    if (!ordered(p.min_end, p.min_start))
        return fail(AFSK_E_INVALID_ARG, "level: 0 <= min_end <= min_start <= 65535 must hold");
    if (p.decay_shift < 0 || p.decay_shift > 15 || p.rise_shift < 0 || p.rise_shift > 15)
        return fail(AFSK_E_INVALID_ARG, "level: decay_shift and rise_shift must lie in 0 ... 15");
    return AFSK_OK;
}

// what afsk_live_level and afsk_live_level_reset ask of their receiver
inline int live_level_receiver(const afsk_live* live, const char* entry) {
    if (!live) return fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (live->max_payload_len < 0)
        return fail(AFSK_E_INVALID_ARG, std::string(entry) + ": a stored live receiver has no level tracker");
    if (!live->leveled)
        return fail(AFSK_E_INVALID_ARG, std::string(entry) + " needs a receiver of afsk_live_create_stream_leveled");
    return AFSK_OK;
}

}  // namespace afsk

extern "C" {

int afsk_live_create_stream_leveled(int32_t n_channels, const int32_t* bit_frames_host_or_null,
                                    const int32_t* cand_bit_frames_host, int32_t n_cand, int32_t max_score,
                                    const int32_t* amp_start_host, const int32_t* amp_end_host, int32_t max_payload_len,
                                    int32_t max_chunk_len, int32_t tap, afsk_live** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (n_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (n_cand < 0 || n_cand > afsk::kLiveAutoMaxCand)
        return afsk::fail(AFSK_E_INVALID_ARG, "n_cand must be 0 ... AFSK_DETECT_MAX_CANDIDATES");
    if (tap != 0 && tap != 1) return afsk::fail(AFSK_E_INVALID_ARG, "tap must be 0 or 1");
    if (!amp_start_host || !amp_end_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const bool is_auto = n_cand > 0;
    // the rates: the candidates of an auto receiver (no channel has one of its own), else one per channel
    const int32_t* rates = is_auto ? cand_bit_frames_host : bit_frames_host_or_null;
    const int32_t n_rates = is_auto ? n_cand : n_channels;
    if (!rates) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t k = 0; k < n_rates; k++)
        if (!afsk::bf_valid(rates[k])) return afsk::fail_bit_frames();
    int32_t cap = 0;
    if (tap)
        if (int rc = afsk::live_tap_cap(n_channels, max_payload_len, max_chunk_len,
                                        *std::min_element(rates, rates + n_rates), cap))
            return rc;
    return afsk::no_throw([&] {
        const std::vector<int32_t> none((size_t)n_channels, 0);
        // per_channel whatever the pairs are: the tracker's output is the two arrays the PER_CHANNEL cells read
        if (int rc = live_create({"afsk_live_create_stream_leveled", n_channels, is_auto ? none.data() : rates, true,
                                  amp_start_host, amp_end_host, true, true, 0, max_payload_len, max_chunk_len}, out))
            return rc;
        afsk_live& lv = **out;
        lv.leveled = true;
        lv.tap_cap = cap;
        if (is_auto) {
            lv.auto_n_cand = n_cand;
            lv.auto_max_score = max_score < 0 ? -1 : max_score;
            std::copy(rates, rates + n_cand, lv.auto_cand);
        }
        return AFSK_OK;
    });
}

int afsk_live_level_check(afsk_live_level_params params) { return afsk::live_level_check(params); }

int afsk_live_level(afsk_live* live, int32_t* d_state, afsk_live_level_params params, const int16_t* chunk,
                    int64_t chunk_row_stride, int32_t chunk_len, const int32_t* d_chunk_lens_or_null,
                    const int32_t* d_mute_or_null, void* hip_stream) {
    if (int rc = afsk::live_level_receiver(live, "afsk_live_level")) return rc;
    if (!d_state || (chunk_len > 0 && !chunk)) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (chunk_len < 0 || chunk_row_stride < 0) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (chunk_len > live->max_chunk_len)
        return afsk::fail(AFSK_E_INVALID_ARG, "chunk_len exceeds the receiver's max_chunk_len");
    if (int rc = afsk::live_level_check(params)) return rc;
    if (int rc = live->state.check_current()) return rc;
    const int64_t n = live->L.n;
    if (n == 0 || chunk_len == 0) return AFSK_OK;                  // no block to walk: the rows and the pair stay
    uint8_t* d = live->state.ptr();
    afsk::LiveLevelArgs a{};
    a.chan = reinterpret_cast<const afsk::LiveChan*>(d);
    a.carry = reinterpret_cast<const int16_t*>(d + live->SL.o_carry);
    a.chunk = chunk;
    a.chunk_stride = chunk_row_stride;
    a.chunk_lens = d_chunk_lens_or_null;
    a.mute = d_mute_or_null;
    a.state = d_state;
    a.thr_start = reinterpret_cast<int32_t*>(d + live->o_thr);
    a.thr_end = a.thr_start + n;
    a.chunk_len = chunk_len;
    a.n = (int32_t)n;
    a.p = params;
    hipLaunchKernelGGL(afsk::live_level_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_level_kernel");
}

int afsk_live_level_reset(afsk_live* live, int32_t* d_state, const uint8_t* d_mask_or_null, int32_t amp_start0,
                          int32_t amp_end0, void* hip_stream) {
    if (int rc = afsk::live_level_receiver(live, "afsk_live_level_reset")) return rc;
    if (!d_state) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = live->state.check_current()) return rc;
    const int64_t n = live->L.n;
    int32_t* thr = reinterpret_cast<int32_t*>(live->state.ptr() + live->o_thr);
    hipLaunchKernelGGL(afsk::live_level_reset_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)hip_stream, d_state, thr, thr + n, d_mask_or_null, (int32_t)n, amp_start0, amp_end0);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_level_reset_kernel");
}

}  // extern "C"
