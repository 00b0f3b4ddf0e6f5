// afsk_live.hip -- the live receiver (afsk_live_*, include/afsk_amd.h): Receiver.receive (afskmodem.py:299-319,
// 402-417) for many channels fed chunk by chunk, with nothing but device state carried from one push to the next.
//
// A push (afsk_live_push.hip: the one kernel template and host path of every receiver's push) is two launches, in
// order on the caller's stream (a captured graph of them is a linear chain):
//   live_push_kernel     its LiveStoreSink cells, one wave per channel: walks the push's whole 2048-sample blocks
//                        through gate_scan_kernel's state machine (discard one block, wait for amp > amp_start,
//                        record through the first amp < amp_end), stores recorded blocks from registers into the
//                        channel's record row, and lays every burst the push closes out as a fixed demodulator slot
//                        (row offset + length).
//   demod_uniform_kernel afsk::launch_demod_uniform over n_channels * slots slots, reading the bursts in place
//                        (length 0 = unused or overflowed slot: status TOO_SHORT, nothing read).
//
// A mixed receiver (afsk_live_create_mixed: a bit_frames per channel) runs the same gate; slot s belongs to channel
// s / slots, so every slot's rate is known at creation, and the second launch is afsk_demod_batch_grouped over the
// slots with a group plan the receiver builds then (the per-stream kernel in rate-sorted order; DESIGN.md 8.2 has
// the measurement against the per-stream kernel in slot order).
//
// A receiver with a threshold pair per channel (afsk_live_create_thresholds) keeps amp_start and amp_end as int32 [n]
// behind the layout's bytes; its gate (the PER_CHANNEL cells, the same walk) takes a channel's pair from there.  The
// demod kernels take one amp_end per launch, so such a receiver launches them once per distinct amp_end -- a squelch
// class, at most AFSK_LIVE_MAX_SQUELCH_CLASSES -- each over the list of that class's slots (DemodArgs::stream_index):
// 1 + classes launches, still nothing on the host in between.  One class (distinct amp_start only) keeps the second
// launch above.  SquelchClasses builds the lists at creation.
//
// Per channel the device keeps (LiveChan) the gate mode, the stream position, the open burst's start, length and
// row offset, and a 2048-sample carry with the partial block at the end of the stream.  Row layout: the open
// burst's prefix at the front, then every block recorded in this push, bursts back to back; at the start of the
// next push a burst that opened in the previous one (behind bursts that closed there) is moved to the front -- at
// most one push's blocks, front to back (the source lies at least one block above the destination).  So a row needs
// cap_blocks (the longest burst that is stored) + k_blocks (the most blocks one push walks) blocks.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end): it uses that
// file's kListenBlock, vec16 and block_abs_sum.
#include <algorithm>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/afsk_amd.h"
#include "afsk_capi_internal.h"

namespace afsk {

struct LiveChan {           // 32 bytes per channel
    int64_t pos;            // samples of the current stream pushed so far; the carry holds the last pos & 2047
    int64_t rec_start;      // open burst: stream index of its first sample
    int64_t rec_len;        // open burst: samples recorded so far (whole blocks; may exceed the row's capacity)
    int32_t mode;           // 0 = discard the next block, 1 = wait for a start block, 2 = recording
    int32_t head;           // open burst: row offset of its first stored sample (0 unless it opened in the
                            // previous push behind bursts that closed there; moved to 0 by the next push)
};
static_assert(sizeof(LiveChan) == 32, "LiveChan layout");

// burst_len is int32: a burst recorded for longer than this (about 12 hours) is reported with this length
constexpr int64_t kLiveLenMax = (int64_t)0x7fffffff & ~(int64_t)(kListenBlock - 1);

struct LiveLayout {
    int64_t n = 0;
    int64_t cap_blocks = 0;     // blocks of a burst that are stored: max_burst_len / 2048
    int64_t k_blocks = 0;       // most blocks one push walks: (2047 + max_chunk_len) / 2048
    int64_t slots = 0;          // slots per channel and push: 1 + k_blocks / 3
    int64_t row_len = 0;        // samples per record row: (cap_blocks + k_blocks) * 2048
    int64_t o_carry = 0, o_slot_off = 0, o_slot_len = 0, o_rows = 0, bytes = 0;
};

// the streaming receiver's (afsk_live_stream.hip: live_stream_layout); here because afsk_live keeps one
struct LiveStreamLayout {
    int64_t n = 0, slots = 0, max_payload = 0;
    int64_t o_carry = 0, o_demod = 0, o_bf = 0, o_win = 0, o_pay = 0, bytes = 0;
};

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

__host__ __device__ inline int64_t min64(int64_t x, int64_t y) { return x < y ? x : y; }

// The state allocation: LiveChan [n] | carry int16 [n, 2048] | slot offset int64 [n, slots] | slot length int32
// [n, slots] | record rows int16 [n, row_len] | 256 spare bytes; every part 256-byte aligned.
inline int live_layout(int32_t n_channels, int32_t max_burst_len, int32_t max_chunk_len, LiveLayout& L) {
    if (n_channels < 1) return fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (max_burst_len < 2 * kListenBlock || max_burst_len > kMaxStreamLen)
        return fail(AFSK_E_INVALID_ARG, "max_burst_len must lie in 4096 ... AFSK_MAX_STREAM_LEN");
    if (max_chunk_len < 1 || max_chunk_len > kMaxStreamLen)
        return fail(AFSK_E_INVALID_ARG, "max_chunk_len must lie in 1 ... AFSK_MAX_STREAM_LEN");
    L.n = n_channels;
    L.cap_blocks = max_burst_len / kListenBlock;
    L.k_blocks = ((int64_t)kListenBlock - 1 + max_chunk_len) / kListenBlock;
    L.slots = 1 + L.k_blocks / 3;
    L.row_len = (L.cap_blocks + L.k_blocks) * kListenBlock;
    if (L.n * L.slots > 0x7fffffffll)
        return fail(AFSK_E_INVALID_ARG, "n_channels * slots exceeds the demodulator's int32 stream count");
    L.o_carry = align256(32 * L.n);
    L.o_slot_off = L.o_carry + align256(2 * kListenBlock * L.n);
    L.o_slot_len = L.o_slot_off + align256(8 * L.n * L.slots);
    L.o_rows = L.o_slot_len + align256(4 * L.n * L.slots);
    L.bytes = L.o_rows + align256(2 * L.row_len * L.n) + 256;   // (n < 2^31, row_len < 2^31: no overflow)
    return AFSK_OK;
}

struct LiveArgs {
    LiveChan* chan;
    int16_t* carry;
    int64_t* slot_off;          // demodulator slots: offset from `rows`, length (0 = nothing to decode)
    int32_t* slot_len;
    int16_t* rows;
    const int16_t* chunk;
    int64_t chunk_stride;
    int64_t row_len;
    int64_t cap;                // cap_blocks * 2048: samples of a burst that are stored
    int32_t chunk_len;
    int32_t flush;
    int32_t n;
    int32_t slots;
    int32_t amp_start;
    int32_t amp_end;
    int32_t* out_n_closed;
    int64_t* out_burst_start;
    int32_t* out_burst_len;
    int32_t* out_flags;
};

// one block of the push: samples [b * 2048 - cl, + 2048) of the chunk (b >= 1, or b == 0 without a carry)
__device__ __forceinline__ void live_load_chunk_block(vec16 (&v)[4], const int16_t* p, int lane) {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = __builtin_nontemporal_load(reinterpret_cast<const vec16*>(p + 512 * j + 8 * lane));
}

// block 0 of a push that starts with cl carried samples: carry[0, cl) then chunk[0, 2048 - cl), sample by sample
// (once per push and channel)
__device__ __forceinline__ void live_load_carry_block(vec16 (&v)[4], const int16_t* carry, const int16_t* src, int cl,
                                                      int lane) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = 512 * j + 8 * lane + 2 * k;
            const uint16_t lo = (uint16_t)(i < cl ? carry[i] : src[i - cl]);
            const uint16_t hi = (uint16_t)(i + 1 < cl ? carry[i + 1] : src[i + 1 - cl]);
            v[j][k] = (uint32_t)lo | ((uint32_t)hi << 16);
        }
}

__device__ __forceinline__ void live_zero_block(vec16 (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = vec16{0u, 0u, 0u, 0u};
}

// The muted walk's select: sample i of the block (register v[i / 512][(i & 511) / 2 - 4 * lane], low half for an even
// i) is column col0 + i of the chunk; the samples whose column lies in [lo, hi) become 0.  One per-lane value, the
// lane's first column relative to lo, and the wave-uniform width hi - lo: sample i is muted iff (uint32)(base + i) <
// width, i a compile-time constant per register half.
__device__ __forceinline__ void live_mute_block(vec16 (&v)[4], int32_t col0, int32_t lo, int32_t hi, int lane) {
    const uint32_t base = (uint32_t)(col0 + 8 * lane - lo);
    const uint32_t width = (uint32_t)(hi - lo);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t i = 512u * j + 2u * k;
            uint32_t x = v[j][k];
            if (base + i < width) x &= 0xffff0000u;
            if (base + i + 1u < width) x &= 0x0000ffffu;
            v[j][k] = x;
        }
}

// The gate walk both live receivers share: one wave per channel walks the push's whole blocks through the listen state
// machine with the next block's load in flight, and hands every event to its sink -- the stored receiver's
// (LiveStoreSink: record rows and demodulator slots) or the streaming one's (afsk_live_stream.hip: demodulation as
// the blocks arrive).  A sink has:
//   Args, Sink(const Args&), gate(const Args&)  the kernel argument it is built from, and the LiveArgs inside that
//   init(a, c, amp_end)           the channel's state is loaded (amp_end: the channel's squelch threshold)
//   begin(a, lane, st)            before the first block
//   overflowed(a, st)             the burst being reported is longer than the sink keeps
//   slot(a, i, c, st, ovf)        lane 0, for every reported burst: the sink's per-slot outputs
//   report(a, i, st, ovf, flags, lane)  every lane, for every reported burst (after slot)
//   start(st)                     a burst opens with the current block
//   record(a, st, cur, lane)      the current block belongs to the open burst (st.rec_len: samples before it)
//   head(st)                      LiveChan::head for the next push (not flushed)
//   finish(a, c, st, lane)        after the walk and the carry, before the unused slots are written
//   clear(a, slot0, i)            unused slot slot0 + i: the sink's own outputs
// PER_CHANNEL: the thresholds are channel c's entries of thr_start / thr_end (int32 [n] in the receiver's state) instead
// of a.amp_start / a.amp_end.  One wave walks one channel, so they are wave-uniform: two scalar loads before the block
// loop, the values in SGPRs for the whole walk.  The instantiations without the flag are the code they were.
// RAGGED (afsk_live_push_ragged): the channel takes len = clamp(chunk_lens[c], 0, a.chunk_len) samples of its row (a null
// chunk_lens: a.chunk_len) and flushes when a.flush or flush_mask[c] is set (a null flush_mask: a.flush alone) -- two
// more wave-uniform scalar loads, walked with in place of a.chunk_len and a.flush.  Nothing at or beyond column len
// of the row is read: the push walks nblk = (cl + len) / 2048 whole blocks (cl: carried samples), block b >= 1 is
// columns [b * 2048 - cl, + 2048) and ends at nblk * 2048 - cl <= len, block 0 of a push with a carry takes its columns
// [0, 2048 - cl) sample by sample (2048 - cl <= len as nblk >= 1), and the carry copy takes columns [nblk * 2048 - cl,
// len).  A channel with len 0 and no flush walks no block, copies nothing, and stores the state it loaded.  The sinks
// never see either value, so plain and ragged pushes of one receiver may alternate.  The instantiations without the
// flag are the code they were.
// MUTE (afsk_live_push_muted, with RAGGED only): columns [lo', hi') of the channel's row count as 0, lo' = clamp(mute[c][0],
// 0, len), hi' = clamp(mute[c][1], lo', len) -- two more wave-uniform scalar loads.  A block whose columns meet the range
// (a wave-uniform test) gets them cleared in its registers before anything uses it (live_mute_block), so the amplitude
// and the sink's record see the zeros; the carry copy stores 0 for a muted column, so a muted sample is 0 in the next
// push too.  Block 0 of a push with a carry goes the same way: its carried samples lie at columns below 0, which no
// range holds, so they are not muted again.  No column at or beyond len is read, as in the ragged form.  Beyond what
// the rule needs, a block that lies wholly inside the range is not loaded: its registers are set to zero, and neither
// the select nor the amplitude sum runs for it.  The instantiations without the flag are the code they were.
template <bool PER_CHANNEL = false, bool RAGGED = false, bool MUTE = false, class Sink>
__device__ __forceinline__ void live_gate_walk(const LiveArgs& a, Sink& sk, const int32_t* thr_start = nullptr,
                                               const int32_t* thr_end = nullptr, const int32_t* chunk_lens = nullptr,
                                               const uint8_t* flush_mask = nullptr, const int32_t* mute = nullptr) {
    static_assert(RAGGED || !MUTE, "the muted walk is a ragged one");
    const int lane = threadIdx.x & 63;
    const int c_lane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c_lane >= a.n) return;
    // MUTE: the channel number as the wave-uniform value it is, so the addresses derived from it (the state, the carry,
    // the outputs) have scalar bases instead of pairs of VGPRs held across the walk -- what keeps the stored cell
    // inside its ragged twin's register allocation.  The other forms keep the per-lane value: the code they were.
    const int c = MUTE ? __builtin_amdgcn_readfirstlane(c_lane) : c_lane;
    LiveChan st = a.chan[c];
    int32_t amp_start = a.amp_start, amp_end = a.amp_end;
    if constexpr (PER_CHANNEL) {
        const int cu = __builtin_amdgcn_readfirstlane(c);
        amp_start = __builtin_amdgcn_readfirstlane(thr_start[cu]);
        amp_end = __builtin_amdgcn_readfirstlane(thr_end[cu]);
    }
    int32_t rag_len = 0, rag_flush = 0;                            // RAGGED: the channel's own length and flush bit
    if constexpr (RAGGED) {
        const int cu = __builtin_amdgcn_readfirstlane(c);
        rag_len = a.chunk_len;
        if (chunk_lens) {
            const int32_t l = __builtin_amdgcn_readfirstlane(chunk_lens[cu]);
            rag_len = l < 0 ? 0 : (l > a.chunk_len ? a.chunk_len : l);
        }
        rag_flush = a.flush;
        if (flush_mask) rag_flush |= __builtin_amdgcn_readfirstlane((int32_t)flush_mask[cu]);
    }
    int32_t mute_lo = 0, mute_hi = 0;                              // MUTE: the channel's muted columns [lo', hi')
    if constexpr (MUTE) {
        const int cu = __builtin_amdgcn_readfirstlane(c);
        const int32_t lo = __builtin_amdgcn_readfirstlane(mute[2 * (int64_t)cu]);
        const int32_t hi = __builtin_amdgcn_readfirstlane(mute[2 * (int64_t)cu + 1]);
        mute_lo = lo < 0 ? 0 : (lo > rag_len ? rag_len : lo);
        mute_hi = hi < mute_lo ? mute_lo : (hi > rag_len ? rag_len : hi);
    }
    // (the plain form reads LiveArgs where it always did)
    auto len = [&]() -> int32_t {
        if constexpr (RAGGED) return rag_len;
        else return a.chunk_len;
    };
    auto flush = [&]() -> int32_t {
        if constexpr (RAGGED) return rag_flush;
        else return a.flush;
    };
    sk.init(a, c, amp_end);
    int16_t* carry = a.carry + (int64_t)c * kListenBlock;
    const int16_t* src = a.chunk + (int64_t)c * a.chunk_stride;
    const int64_t slot0 = (int64_t)c * a.slots;
    sk.begin(a, lane, st);

    const int cl = (int)(st.pos & (kListenBlock - 1));             // carried samples
    const int32_t nblk = (int32_t)(((int64_t)cl + len()) / kListenBlock);
    const int64_t bpos0 = st.pos - cl;                              // stream index of block 0
    int k = 0;                                                      // slots used
    auto report = [&](int32_t flags) {
        const bool ovf = sk.overflowed(a, st);
        if (k < a.slots && lane == 0) {                             // (k < slots always holds: afsk_live_layout)
            const int64_t i = slot0 + k;
            a.out_burst_start[i] = st.rec_start;
            a.out_burst_len[i] = (int32_t)min64(st.rec_len, kLiveLenMax);
            a.out_flags[i] = flags | (ovf ? AFSK_LIVE_OVERFLOW : 0);
            sk.slot(a, i, c, st, ovf);
        }
        sk.report(a, slot0 + k, st, ovf, flags, lane);
        k++;
    };
    // MUTE: block b lies wholly inside the muted range (wave-uniform; never block 0 of a push with a carry, whose first
    // column is below 0): it is zeros, and its columns are not loaded
    auto mute_whole = [&](int32_t b) -> bool {
        if constexpr (MUTE) {
            const int32_t col0 = b * kListenBlock - cl;
            return mute_lo <= col0 && col0 + kListenBlock <= mute_hi;
        } else {
            return false;
        }
    };
    vec16 cur[4], nxt[4];
    if (nblk > 0) {
        if (cl > 0) live_load_carry_block(cur, carry, src, cl, lane);
        else if (mute_whole(0)) live_zero_block(cur);
        else live_load_chunk_block(cur, src, lane);
    }
    for (int32_t b = 0; b < nblk; b++) {
        if (b + 1 < nblk) {                                         // next block in flight
            if (mute_whole(b + 1)) live_zero_block(nxt);
            else live_load_chunk_block(nxt, src + (int64_t)(b + 1) * kListenBlock - cl, lane);
        }
        const bool whole = mute_whole(b);                           // (zeros already: no select, and no sum to take)
        if constexpr (MUTE) {
            const int32_t col0 = b * kListenBlock - cl;             // the block's first column (< 0: carried samples)
            if (!whole && mute_lo < mute_hi && mute_lo < col0 + kListenBlock && mute_hi > col0)      // wave-uniform
                live_mute_block(cur, col0, mute_lo, mute_hi, lane);
        }
        const int32_t amp = whole ? 0 : (int32_t)((uint32_t)__builtin_amdgcn_readlane(block_abs_sum(cur), 63) >> 11);
        int ev = 0;                                                 // 1 = record the block, 2 = record it and close
        if (st.mode == 0) {
            st.mode = 1;                                            // ref:303
        } else if (st.mode == 1) {
            if (amp > amp_start) {                                  // ref:306-309
                st.mode = 2;
                st.rec_start = bpos0 + (int64_t)b * kListenBlock;
                st.rec_len = 0;
                sk.start(st);
                ev = 1;
            }
        } else {
            ev = amp < amp_end ? 2 : 1;                             // ref:316-318 (block included)
        }
        if (ev) {
            sk.record(a, st, cur, lane);
            st.rec_len += kListenBlock;
            if (ev == 2) {
                report(0);
                st.mode = 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) cur[j] = nxt[j];
    }

    if (flush()) {
        if (st.mode == 2) report(AFSK_LIVE_OPEN_END);               // gate_scan_kernel's open-ended burst
        st = LiveChan{};                                            // a new stream; the partial block is dropped
    } else {
        // the tail (< 2048 samples) to the carry: carry[i] = stream sample nblk * 2048 + i for i < tail; without a
        // whole block in this push only [cl, tail) is new
        const int32_t tail = (int32_t)(((int64_t)cl + len()) & (kListenBlock - 1));
        const int64_t base = (int64_t)nblk * kListenBlock - cl;
        for (int i = (nblk == 0 ? cl : 0) + lane; i < tail; i += 64) {
            if constexpr (MUTE) {
                const int64_t col = base + i;
                carry[i] = col >= mute_lo && col < mute_hi ? (int16_t)0 : src[col];
            } else {
                carry[i] = src[base + i];
            }
        }
        st.pos += len();
        st.head = sk.head(st);
    }
    sk.finish(a, c, st, lane);
    for (int i = k + lane; i < a.slots; i += 64) {                  // unused slots: length 0, nothing to decode
        a.out_burst_start[slot0 + i] = 0;
        a.out_burst_len[slot0 + i] = 0;
        a.out_flags[slot0 + i] = 0;
        sk.clear(a, slot0, i);
    }
    if (lane == 0) {
        a.out_n_closed[c] = k < a.slots ? k : a.slots;
        a.chan[c] = st;
    }
}

// The stored receiver's sink: recorded blocks go from registers into the channel's record row, and every burst the
// push closes becomes a demodulator slot (row offset + length) for the push's second launch.
struct LiveStoreSink {
    using Args = LiveArgs;      // what live_push_kernel (afsk_live_push.hip) hands the sink, and the gate's part of it
    int16_t* row;
    int64_t wp;                 // row offset of the next stored block
    int64_t brow;               // row offset of the open burst

    __device__ __forceinline__ explicit LiveStoreSink(const Args&) {}
    static __device__ __forceinline__ const LiveArgs& gate(const Args& a) { return a; }

    // the open burst's stored prefix goes to the row front (it opened in the previous push behind closed bursts,
    // so it is at most one push of blocks, and head >= 2048: copying block by block front to back never overwrites
    // a block that is still to be read)
    __device__ __forceinline__ void init(const LiveArgs& a, int c, int32_t) { row = a.rows + (int64_t)c * a.row_len; }
    __device__ __forceinline__ void begin(const LiveArgs& a, int lane, const LiveChan& st) {
        wp = 0;
        brow = 0;
        if (st.mode == 2) {
            const int64_t stored = min64(st.rec_len, a.cap);
            if (st.head > 0)
                for (int64_t o = 0; o < stored; o += kListenBlock) {
                    vec16 v[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = *reinterpret_cast<const vec16*>(row + st.head + o + 512 * j + 8 * lane);
#pragma unroll
                    for (int j = 0; j < 4; j++) *reinterpret_cast<vec16*>(row + o + 512 * j + 8 * lane) = v[j];
                }
            wp = stored;
        }
    }
    __device__ __forceinline__ bool overflowed(const LiveArgs& a, const LiveChan& st) const { return st.rec_len > a.cap; }
    __device__ __forceinline__ void slot(const LiveArgs& a, int64_t i, int c, const LiveChan& st, bool ovf) const {
        a.slot_off[i] = (int64_t)c * a.row_len + brow;
        a.slot_len[i] = ovf ? 0 : (int32_t)st.rec_len;
    }
    __device__ __forceinline__ void report(const LiveArgs&, int64_t, const LiveChan&, bool, int32_t, int) const {}
    __device__ __forceinline__ void start(const LiveChan&) { brow = wp; }
    __device__ __forceinline__ void record(const LiveArgs& a, const LiveChan& st, const vec16 (&cur)[4], int lane) {
        // stored while the burst fits its capacity (and, as a guard, the row)
        if (st.rec_len < a.cap && wp + kListenBlock <= a.row_len) {
#pragma unroll
            for (int j = 0; j < 4; j++) *reinterpret_cast<vec16*>(row + wp + 512 * j + 8 * lane) = cur[j];
            wp += kListenBlock;
        }
    }
    __device__ __forceinline__ int32_t head(const LiveChan& st) const { return st.mode == 2 ? (int32_t)brow : 0; }
    __device__ __forceinline__ void finish(const LiveArgs&, int, const LiveChan&, int) const {}
    __device__ __forceinline__ void clear(const LiveArgs& a, int64_t slot0, int i) const {
        a.slot_off[slot0 + i] = 0;
        a.slot_len[slot0 + i] = 0;
    }
};

__global__ __launch_bounds__(256) void live_reset_kernel(LiveChan* chan, const uint8_t* mask, int32_t n) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n && (!mask || mask[c])) chan[c] = LiveChan{};
}

// afsk_live_busy: busy[c] = 1 while channel c's gate is recording a burst (every receiver kind keeps LiveChan [n] at
// the front of its state)
__global__ __launch_bounds__(256) void live_busy_kernel(const LiveChan* chan, int32_t* busy, int32_t n) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n) busy[c] = chan[c].mode == 2 ? 1 : 0;
}

}  // namespace afsk

namespace afsk {

// The stored receiver's squelch classes (afsk_live_create_thresholds).  The demod kernels take ONE amp_end per launch,
// and a launch decodes the streams its stream_index lists: the channels are grouped by distinct amp_end (a class, in
// order of first appearance), and a class's list holds its demodulator slots c * slots + k in ascending order -- for
// a class of four or more rates sorted by rate inside windows of 4096 entries, the order a group plan walks a batch in
// (neighbouring waves run one rate's code; a different order changes speed, never results).  Every slot is in
// exactly one list, so the class launches of a push write every output row exactly once.
struct SquelchClasses {
    struct Class {
        int32_t amp_end;
        int32_t first, count;       // its part of `list`
        int32_t uniform_bf;         // the one bit_frames of its channels, 0 when they differ
    };
    std::vector<Class> classes;
    std::vector<int32_t> list;      // [n * slots], class after class

    // host only; bit_frames: [n] or null with `uniform_bf` for every channel.  One pass over the channels: a channel
    // joins the class of its amp_end or opens the next one (the caller has checked how many there are), so classes come
    // in order of first appearance with their channels ascending.
    void build(int32_t n, int32_t slots, const int32_t* bit_frames, int32_t uniform_bf, const int32_t* amp_end) {
        classes.clear();
        std::vector<std::vector<int32_t>> chans;
        for (int32_t c = 0; c < n; c++) {
            size_t k = 0;
            while (k < classes.size() && classes[k].amp_end != amp_end[c]) k++;
            if (k == classes.size()) {
                classes.push_back({amp_end[c], 0, 0, 0});
                chans.emplace_back();
            }
            chans[k].push_back(c);
        }
        list.clear();
        list.reserve((size_t)n * (size_t)slots);
        for (size_t k = 0; k < classes.size(); k++) {
            Class& cl = classes[k];
            cl.first = (int32_t)list.size();
            std::vector<int32_t> rates;
            for (int32_t c : chans[k]) {
                const int32_t bf = bit_frames ? bit_frames[c] : uniform_bf;
                if (std::find(rates.begin(), rates.end(), bf) == rates.end()) rates.push_back(bf);
                for (int32_t j = 0; j < slots; j++) list.push_back(c * slots + j);
            }
            cl.count = (int32_t)list.size() - cl.first;
            cl.uniform_bf = rates.size() == 1 ? rates[0] : 0;
            if (rates.size() >= 4)      // (windows counted from the class's first entry)
                for (int32_t w0 = cl.first; w0 < cl.first + cl.count; w0 += 4096)
                    std::stable_sort(list.begin() + w0, list.begin() + std::min(w0 + 4096, cl.first + cl.count),
                                     [&](int32_t x, int32_t y) { return bit_frames[x / slots] < bit_frames[y / slots]; });
        }
    }

    static int32_t count_distinct(const int32_t* amp_end, int32_t n) {
        std::vector<int32_t> v(amp_end, amp_end + n);
        std::sort(v.begin(), v.end());
        return (int32_t)(std::unique(v.begin(), v.end()) - v.begin());
    }
};

}  // namespace afsk

struct afsk_live {
    afsk::DeviceState state;            // the layout's L.bytes (+ the per-channel part of a thresholds receiver)
    afsk::LiveLayout L;
    afsk::LiveStreamLayout SL;          // a streaming receiver's layout (L then holds n and slots only)
    int32_t bit_frames = 0, amp_start = 0, amp_end = 0, max_chunk_len = 0;   // (a mixed receiver: bit_frames 0)
    afsk_group_plan* plan = nullptr;    // mixed: the plan over the slots (8 bytes per slot on the device)
    int32_t max_payload_len = -1;       // >= 0: a streaming receiver (afsk_live_stream.hip)
    int32_t tap_cap = 0;                // > 0: a tapped streaming receiver (afsk_live_tap.hip): bytes per tap row
    // > 0: an auto-rate streaming receiver (afsk_live_auto.hip): the candidate list every push passes by value
    int32_t auto_n_cand = 0, auto_max_score = -1;
    int32_t auto_cand[AFSK_DETECT_MAX_CANDIDATES] = {};
    // a threshold pair per channel (afsk_live_create_thresholds / _stream_thresholds): amp_start int32 [n] at o_thr,
    // amp_end int32 [n] behind it; a stored receiver of two or more squelch classes also the classes' slot lists
    // (o_list: int32 [n * slots]) and, with mixed rates, every slot's bit_frames (o_slot_bf: int32 [n * slots])
    bool per_channel = false;
    bool leveled = false;               // afsk_live_create_stream_leveled: afsk_live_level may rewrite the pair arrays
    int64_t o_thr = 0, o_list = 0, o_slot_bf = 0;
    std::vector<afsk::SquelchClasses::Class> classes;     // (one class: today's demod launch, no list)
    ~afsk_live() {
        if (plan) (void)afsk_group_plan_destroy(plan);
    }
    const int32_t* thr_start() const { return reinterpret_cast<const int32_t*>(state.ptr() + o_thr); }
    const int32_t* thr_end() const { return thr_start() + L.n; }
};

namespace afsk {
// the streaming receiver's reset (afsk_live_stream.hip), after afsk_live_reset's checks
int live_stream_reset(afsk_live* live, const uint8_t* d_mask_or_null, hipStream_t stream);

// What a create entry asks for, after its own argument checks.  bit_frames: [n] when `mixed`, else bit_frames[0] for
// every channel; amp_start / amp_end: [n] when `per_channel`, else [0] for every channel.  `streaming`: the
// streaming receiver with max_payload_len (else the stored one with max_burst_len).
struct LiveSpec {
    const char* entry;
    int32_t n_channels;
    const int32_t* bit_frames;
    bool mixed;
    const int32_t* amp_start;
    const int32_t* amp_end;
    bool per_channel;
    bool streaming;
    int32_t max_burst_len, max_payload_len, max_chunk_len;
};

// the streaming receiver's layout and state (afsk_live_stream.hip), inside live_create
int live_stream_state(const LiveSpec& sp, afsk_live& lv);
}  // namespace afsk

namespace afsk {

// the stored receiver's second launch (or launches, one per squelch class): the demodulator over the slots
int live_stored_demod(afsk_live* live, const LiveArgs& g, const DemodOutputs& o, hipStream_t st) {
    const LiveLayout& L = live->L;
    uint8_t* d = live->state.ptr();
    hipError_t e;
    // an unused slot reports 0 corrected codewords; once for all classes, which share the arrays through their index
    // lists (the grouped entry below clears them itself)
    if (!live->classes.empty() || !live->plan)
        if (int rc = clear_corrected(o.corrected, L.n * L.slots, st)) return rc;
    // two or more squelch classes: the demod kernels once per class, each over its own list of slots
    for (const SquelchClasses::Class& k : live->classes) {
        DemodArgs a = o.args<DemodArgs>(g.rows, g.slot_off, g.slot_len, k.amp_end, k.count);
        a.stream_index = reinterpret_cast<const int32_t*>(d + live->o_list) + k.first;
        if (k.uniform_bf) {
            a.uniform_bit_frames = k.uniform_bf;
            e = launch_demod_uniform(a, st);
        } else {
            a.bit_frames = reinterpret_cast<const int32_t*>(d + live->o_slot_bf);
            e = launch_demod(a, st);
        }
        if (e != hipSuccess) return hip_fail(e, "launch the demod kernel (live slots of one squelch class)");
    }
    if (!live->classes.empty()) return AFSK_OK;
    if (live->plan)
        return afsk_demod_batch_grouped(live->plan, g.rows, g.slot_off, g.slot_len, live->amp_end, o.bytes, o.stride,
                                        o.nbytes, o.nbits, o.clock_idx, o.term_frame, o.status, o.corrected,
                                        o.margins, o.margin_stride, st);
    DemodArgs a = o.args<DemodArgs>(g.rows, g.slot_off, g.slot_len, live->amp_end, (int32_t)(L.n * L.slots));
    a.uniform_bit_frames = live->bit_frames;
    e = launch_demod_uniform(a, st);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch demod_uniform_kernel (live slots)");
}

}  // namespace afsk

extern "C" {

int afsk_live_layout(int32_t n_channels, int32_t max_burst_len, int32_t max_chunk_len, int32_t* out_slots,
                     int64_t* out_state_bytes) {
    afsk::LiveLayout L;
    if (int rc = afsk::live_layout(n_channels, max_burst_len, max_chunk_len, L)) return rc;
    if (out_slots) *out_slots = (int32_t)L.slots;
    if (out_state_bytes) *out_state_bytes = L.bytes;
    return AFSK_OK;
}

namespace {

// the stored receiver's layout and state
int live_stored_state(const afsk::LiveSpec& sp, afsk_live& lv) {
    const afsk::LiveLayout& L = lv.L;
    if (int rc = afsk::live_layout(sp.n_channels, sp.max_burst_len, sp.max_chunk_len, lv.L)) return rc;
    lv.bit_frames = sp.mixed ? 0 : sp.bit_frames[0];
    const int64_t n_slots = L.n * L.slots;
    bool plan = sp.mixed;
    int64_t bytes = L.bytes;
    std::vector<int32_t> tail;                  // what follows the layout's bytes, as int32
    if (sp.per_channel) {
        afsk::SquelchClasses sc;
        sc.build(sp.n_channels, (int32_t)L.slots, sp.mixed ? sp.bit_frames : nullptr, sp.bit_frames[0], sp.amp_end);
        const int64_t thr = afsk::align256(4 * L.n) / 4;
        const int64_t per_slot = afsk::align256(4 * n_slots) / 4;
        const bool lists = sc.classes.size() > 1;
        lv.o_thr = L.bytes;
        tail.assign((size_t)(2 * thr + (lists ? per_slot : 0) + (lists && sp.mixed ? per_slot : 0)), 0);
        // (amp_end directly behind amp_start: afsk_live::thr_end)
        std::copy(sp.amp_start, sp.amp_start + L.n, tail.begin());
        std::copy(sp.amp_end, sp.amp_end + L.n, tail.begin() + L.n);
        if (lists) {
            lv.o_list = lv.o_thr + 8 * thr;
            std::copy(sc.list.begin(), sc.list.end(), tail.begin() + 2 * thr);
            if (sp.mixed) {
                lv.o_slot_bf = lv.o_list + 4 * per_slot;
                for (int64_t s = 0; s < n_slots; s++) tail[(size_t)(2 * thr + per_slot + s)] = sp.bit_frames[s / L.slots];
            }
            lv.classes = sc.classes;
            plan = false;                       // the class launches walk their own lists
        } else {
            lv.amp_end = sc.classes[0].amp_end;
        }
        bytes += 4 * (int64_t)tail.size();
    }
    // only the channel states need a value: the carry, slots and rows are written before they are read
    if (int rc = lv.state.create(sp.entry, bytes, L.o_carry, tail.empty() ? nullptr : tail.data(), lv.o_thr,
                                 4 * (int64_t)tail.size()))
        return rc;
    if (plan) {
        std::vector<int32_t> slot_bf((size_t)n_slots);
        for (size_t s = 0; s < slot_bf.size(); s++) slot_bf[s] = sp.bit_frames[(int64_t)s / L.slots];
        if (int rc = afsk_group_plan_create(slot_bf.data(), (int32_t)slot_bf.size(), &lv.plan)) return rc;
    }
    return AFSK_OK;
}

// Every create entry, after its own argument checks: the one owner of a receiver's host fields and device state.
int live_create(const afsk::LiveSpec& sp, afsk_live** out) {
    return afsk::no_throw([&] {
        std::unique_ptr<afsk_live> lv(new afsk_live());
        lv->amp_start = sp.amp_start[0];
        lv->amp_end = sp.amp_end[0];
        lv->per_channel = sp.per_channel;
        lv->max_chunk_len = sp.max_chunk_len;
        if (int rc = sp.streaming ? afsk::live_stream_state(sp, *lv) : live_stored_state(sp, *lv)) return rc;
        *out = lv.release();
        return AFSK_OK;
    });
}

// The checks the array entries share; `same`: every channel at one rate.
int live_check_rates(int32_t n_channels, const int32_t* bit_frames_host, afsk_live** out, bool& same) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (n_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (!bit_frames_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    same = true;
    for (int32_t c = 0; c < n_channels; c++) {
        if (!afsk::bf_valid(bit_frames_host[c])) return afsk::fail_bit_frames();
        same = same && bit_frames_host[c] == bit_frames_host[0];
    }
    return AFSK_OK;
}

bool all_equal(const int32_t* v, int32_t n) {
    for (int32_t c = 1; c < n; c++)
        if (v[c] != v[0]) return false;
    return true;
}

}  // namespace

int afsk_live_create(int32_t n_channels, int32_t bit_frames, int32_t amp_start_threshold, int32_t amp_end_threshold,
                     int32_t max_burst_len, int32_t max_chunk_len, afsk_live** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (!afsk::bf_valid(bit_frames)) return afsk::fail_bit_frames();
    return live_create({"afsk_live_create", n_channels, &bit_frames, false, &amp_start_threshold, &amp_end_threshold,
                        false, false, max_burst_len, -1, max_chunk_len}, out);
}

int afsk_live_create_mixed(int32_t n_channels, const int32_t* bit_frames_host, int32_t amp_start_threshold,
                           int32_t amp_end_threshold, int32_t max_burst_len, int32_t max_chunk_len, afsk_live** out) {
    bool same;
    if (int rc = live_check_rates(n_channels, bit_frames_host, out, same)) return rc;
    // one rate for every channel: the uniform receiver (its launches, its state bytes)
    return live_create({"afsk_live_create", n_channels, bit_frames_host, !same, &amp_start_threshold,
                        &amp_end_threshold, false, false, max_burst_len, -1, max_chunk_len}, out);
}

int afsk_live_create_thresholds(int32_t n_channels, const int32_t* bit_frames_host, const int32_t* amp_start_host,
                                const int32_t* amp_end_host, int32_t max_burst_len, int32_t max_chunk_len,
                                afsk_live** out) {
    bool same;
    if (int rc = live_check_rates(n_channels, bit_frames_host, out, same)) return rc;
    if (!amp_start_host || !amp_end_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    return afsk::no_throw([&] {
        if (afsk::SquelchClasses::count_distinct(amp_end_host, n_channels) > AFSK_LIVE_MAX_SQUELCH_CLASSES)
            return afsk::fail(AFSK_E_INVALID_ARG,
                              "more than AFSK_LIVE_MAX_SQUELCH_CLASSES (16) distinct amp_end thresholds on a stored live "
                              "receiver (one demod launch each): the streaming receiver, "
                              "afsk_live_create_stream_thresholds, has no such limit");
        // one pair for every channel: the receiver afsk_live_create_mixed builds
        const bool per_channel = !all_equal(amp_start_host, n_channels) || !all_equal(amp_end_host, n_channels);
        return live_create({"afsk_live_create_thresholds", n_channels, bit_frames_host, !same, amp_start_host,
                            amp_end_host, per_channel, false, max_burst_len, -1, max_chunk_len}, out);
    });
}

int afsk_live_squelch_classes(int32_t n_channels, int32_t slots, const int32_t* bit_frames_host,
                              const int32_t* amp_end_host, int32_t* out_n_classes, int32_t* out_class_amp_end,
                              int32_t* out_class_count, int32_t* out_class_uniform_bf, int32_t* out_slot_list) {
    if (n_channels < 1 || slots < 1 || (int64_t)n_channels * slots > 0x7fffffffll)
        return afsk::fail(AFSK_E_INVALID_ARG, "n_channels and slots must be at least 1, their product an int32");
    if (!bit_frames_host || !amp_end_host || !out_n_classes) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    return afsk::no_throw([&] {
        const int32_t nd = afsk::SquelchClasses::count_distinct(amp_end_host, n_channels);
        *out_n_classes = nd;
        if (nd > AFSK_LIVE_MAX_SQUELCH_CLASSES)
            return afsk::fail(AFSK_E_INVALID_ARG, "more than AFSK_LIVE_MAX_SQUELCH_CLASSES (16) distinct amp_end thresholds");
        afsk::SquelchClasses sc;
        sc.build(n_channels, slots, bit_frames_host, 0, amp_end_host);
        for (size_t k = 0; k < sc.classes.size(); k++) {
            if (out_class_amp_end) out_class_amp_end[k] = sc.classes[k].amp_end;
            if (out_class_count) out_class_count[k] = sc.classes[k].count;
            if (out_class_uniform_bf) out_class_uniform_bf[k] = sc.classes[k].uniform_bf;
        }
        if (out_slot_list) std::copy(sc.list.begin(), sc.list.end(), out_slot_list);
        return AFSK_OK;
    });
}

int afsk_live_info(const afsk_live* live, int32_t* out_n_channels, int32_t* out_slots, int64_t* out_state_bytes) {
    if (!live) return afsk::fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (out_n_channels) *out_n_channels = (int32_t)live->L.n;
    if (out_slots) *out_slots = (int32_t)live->L.slots;
    if (out_state_bytes) *out_state_bytes = live->state.bytes + (live->plan ? 8 * live->L.n * live->L.slots : 0);
    return AFSK_OK;
}

int afsk_live_reset(afsk_live* live, const uint8_t* d_mask_or_null, void* hip_stream) {
    if (!live) return afsk::fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (int rc = live->state.check_current()) return rc;
    if (live->max_payload_len >= 0) return afsk::live_stream_reset(live, d_mask_or_null, (hipStream_t)hip_stream);
    hipLaunchKernelGGL(afsk::live_reset_kernel, dim3((uint32_t)((live->L.n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)hip_stream, static_cast<afsk::LiveChan*>(live->state.d), d_mask_or_null,
                       (int32_t)live->L.n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_reset_kernel");
}

int afsk_live_busy(afsk_live* live, int32_t* d_out_busy, void* hip_stream) {
    if (!live) return afsk::fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (!d_out_busy) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = live->state.check_current()) return rc;
    hipLaunchKernelGGL(afsk::live_busy_kernel, dim3((uint32_t)((live->L.n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)hip_stream, static_cast<const afsk::LiveChan*>(live->state.d), d_out_busy,
                       (int32_t)live->L.n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_busy_kernel");
}

int afsk_live_destroy(afsk_live* live) {
    delete live;      // the caller has synchronised the launches that use it
    return AFSK_OK;
}

}  // extern "C"
