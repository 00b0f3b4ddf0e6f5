// afsk_live_stream.hip -- the streaming live receiver (afsk_live_stream_layout / afsk_live_create_stream,
// include/afsk_amd.h): the stored receiver's gate, slots and outputs, with every burst demodulated WHILE its blocks are
// gated.  No samples of a burst are kept beyond what the next push needs, so burst length has no cap and the state per
// channel does not depend on it.
//
// A push is ONE launch: live_push_kernel (afsk_live_push.hip) runs live_gate_walk (afsk_live.hip) with LiveStreamSink.
// For every block the gate records into a burst, the sink writes the block from registers into the wave's two-block
// LDS window (burst block j in half j & 1, so the window holds sample p of the burst at p & 4095) and moves the
// burst's demodulator on:
//   block 0        nothing more (the clock index needs the first 4096 samples)
//   block 1        clock recovery on the window (split_clock_kernel's helpers: clock_index_is_zero /
//                  recover_clock_index_lanes at bit_frames 40, recover_clock_index_rt otherwise)
//   every block    the symbols k with ci + (k + 1) * bf < len (len: samples recorded so far) that are not committed yet
//                  -- split_finish_kernel's K rule, so a symbol that ends at the last sample waits for the next block:
//                  a symbol (bf <= 2000) spans at most two blocks.  Decisions and loud flags by
//                  split_segment_rt_kernel's quarter sums, lps = 1, 2, 4 ... 32 lanes per symbol (bf / 32 rounded down
//                  to a power of two, so one pass of 64 lanes covers a block), reduced across the lanes; then the
//                  terminator search, the squelch stop, Hamming decode and byte packing of split_finish_kernel,
//                  incrementally: the last three decisions, the pending coded bits and the high nibble carry over.
// A push ends with the samples the next push needs copied out of the window: the first block while only one is
// recorded, else the uncommitted symbol's samples [ci + k * bf, len) (at most bf).  The next push copies them back.
//
// Per channel the state holds LiveChan and the carry (as the stored receiver), StreamDemod (32 B), its bit_frames, a
// 4096-sample window image and a payload row of max_payload_len bytes.  A reported burst's outputs come from
// StreamDemod and the payload row (bytes [0, min(nbytes, max_payload_len, out_stride)) are copied into its row).
//
// A receiver with a threshold pair per channel (afsk_live_create_stream_thresholds) keeps amp_start and amp_end as
// int32 [n] behind bit_frames; the PER_CHANNEL cells of live_push_kernel (the same walk and sink) gate with the
// channel's pair and set the sink's per-symbol squelch from the channel's amp_end -- any number of distinct pairs,
// still one launch.
//
// A tapped receiver (afsk_live_tap.hip: afsk_live_create_stream_tap, afsk_live_push_tap) is this receiver with the same
// state; its push runs the sink's tapped instantiation (LiveStreamSinkT<true>), which also hands out every payload
// byte in the push that commits it.
//
// The auto-rate receiver (afsk_live_auto.hip: afsk_live_create_stream_auto, afsk_live_push_auto) is this receiver with
// the same state and a sink derived from this one: the sink's steps (set_rate, rows, put, clock, lock, symbols) are
// members of their own so that it can decide a burst's rate between put and lock; StreamDemod::spare holds that rate.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), after afsk_split.hip
// (the demod helpers) and afsk_live.hip (the gate walk, LiveChan, LiveArgs).

namespace afsk {

struct StreamDemod {        // 32 bytes per channel: the open burst's demodulator
    int32_t phase;          // 0 = fewer than 4096 samples, 1 = terminator search, 2 = data, 3 = stopped
    int32_t ci;             // clock index (phase >= 1)
    int32_t k;              // next symbol to commit
    int32_t first;          // first data symbol = terminator + 1 (phase >= 2)
    int32_t nbits;          // data bits taken (ref:380)
    int32_t corrected;      // whole codewords with a non-zero syndrome
    uint32_t bits;          // phase 1: the last three decisions (bit 0 = oldest); phase 2: the nbits % 7 pending
                            // coded bits (bit 0 = oldest) | the high nibble of an unfinished byte << 8
    int32_t spare;          // the auto-rate sink (afsk_live_auto.hip): (score << 11) | bit_frames of the open burst
};
static_assert(sizeof(StreamDemod) == 32, "StreamDemod layout");

constexpr int kStreamWin = 2 * kListenBlock;                  // samples in a window
constexpr int kStreamWinLds = 2 * kStreamWin + 128;           // LDS bytes per wave: the window + what the clock
                                                              // searches read past its end (idle lanes, ignored)

// LiveStreamLayout (defined in afsk_live.hip: afsk_live keeps the one its receiver was created with): LiveChan [n] |
// carry int16 [n, 2048] | StreamDemod [n] | bit_frames int32 [n] | window int16 [n, 4096] | payload uint8
// [n, max_payload_len] | 256 spare bytes; every part 256-byte aligned.  `per_channel` (a threshold pair per channel,
// afsk_live_create_stream_thresholds): the bit_frames part holds int32 [3, n] -- bit_frames, amp_start, amp_end.
inline int live_stream_layout(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len, LiveStreamLayout& L,
                              bool per_channel = false) {
    if (n_channels < 1) return fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (max_payload_len < 0 || max_payload_len > 65536)
        return fail(AFSK_E_INVALID_ARG, "max_payload_len must lie in 0 ... 65536");
    if (max_chunk_len < 1 || max_chunk_len > kMaxStreamLen)
        return fail(AFSK_E_INVALID_ARG, "max_chunk_len must lie in 1 ... AFSK_MAX_STREAM_LEN");
    const int64_t k_blocks = ((int64_t)kListenBlock - 1 + max_chunk_len) / kListenBlock;
    L.n = n_channels;
    L.slots = 1 + k_blocks / 3;
    L.max_payload = max_payload_len;
    if (L.n * L.slots > 0x7fffffffll)
        return fail(AFSK_E_INVALID_ARG, "n_channels * slots exceeds the demodulator's int32 stream count");
    L.o_carry = align256(32 * L.n);
    L.o_demod = L.o_carry + align256(2 * kListenBlock * L.n);
    L.o_bf = L.o_demod + align256(32 * L.n);
    L.o_win = L.o_bf + align256((per_channel ? 12 : 4) * L.n);
    L.o_pay = L.o_win + align256(2 * kStreamWin * L.n);
    L.bytes = L.o_pay + align256(L.max_payload * L.n) + 256;
    return AFSK_OK;
}

struct LiveStreamArgs {
    LiveArgs g;                 // the gate's part (rows, slot_off, slot_len, row_len, cap unused)
    StreamDemod* dm;
    const int32_t* bit_frames;
    int16_t* win;
    uint8_t* pay;
    int32_t max_payload;
    uint8_t* out_bytes;
    int32_t out_stride;
    int32_t* out_nbytes;
    int32_t* out_nbits;
    int32_t* out_clock_idx;
    int32_t* out_term_frame;
    int32_t* out_status;
    int32_t* out_corrected;
};

// Decisions (bit i = symbol i) and loud flags of the n <= 64 >> lsh symbols whose first samples sit at burst positions
// s0 + i * bf, from the window: 1 << lsh lanes per symbol, each summing every (1 << lsh)-th sample of it into the
// mark / space combinations of split_segment_rt_kernel's quarter sums and |x|, then a reduction over the group.
__device__ __forceinline__ void stream_symbols(const int16_t* win, int lane, int bf, int lsh, int32_t s0, int n,
                                               uint32_t amp_thr, uint64_t& dec, uint64_t& loud) {
    const int lps = 1 << lsh;
    const int g = lane >> lsh, sub = lane & (lps - 1);
    const bool valid = g < n;
    const int32_t base = s0 + (valid ? g : 0) * bf;            // (idle lanes re-read the first symbol)
    const int q = bf >> 2;
    int32_t sm = 0, ss = 0;                                     // h0 - h1 + h2 - h3, h0 + h1 - h2 - h3
    uint32_t amp = 0;
    int qi = 0, nb = q;                                         // quarter of sample j, its end (lps < q: one step)
    for (int j = sub; j < bf; j += lps) {
        if (j >= nb) { qi++; nb += q; }
        const int32_t x = win[(base + j) & (kStreamWin - 1)];
        const int32_t h = x > 512 ? 0 : (x < -512 ? 65535 : 32767);    // 65535 - limited (ref:287-296), biased
        sm += (qi & 1) ? -h : h;
        ss += (qi & 2) ? -h : h;
        amp += (uint32_t)(x < 0 ? -x : x);                                // ref:94-98
    }
    for (int m = lps >> 1; m > 0; m >>= 1) {
        sm += __shfl_xor(sm, m);
        ss += __shfl_xor(ss, m);
        amp += (uint32_t)__shfl_xor((int)amp, m);
    }
    const uint32_t full = 65535u * (uint32_t)q;
    const uint32_t md = (2u * full + (uint32_t)sm) / (uint32_t)bf, sd = (2u * full + (uint32_t)ss) / (uint32_t)bf;
    int r = (md < sd ? 1 : 0) | (amp >= amp_thr ? 2 : 0);      // ref:348-351, 375
    if (lsh > 0) r = __shfl(r, (lane < n ? lane : 0) << lsh);  // symbol `lane` from its group's first lane
    dec = __ballot(lane < n && (r & 1));
    loud = __ballot(lane < n && (r & 2));
}

// The payload tap (afsk_live_tap.hip: afsk_live_push_tap).  The tapped instantiation of the sink appends every byte it
// commits to the channel's tap row and counts them per reported burst; the untapped one holds and does none of it.
struct LiveTapArgs {
    uint8_t* bytes;             // uint8 [n, cap]: the bytes committed during this push, in time order
    int32_t cap;
    int32_t* n;                 // int32 [n]: how many
    int32_t* len;               // int32 [n, slots]: how many of them belong to the burst of slot (c, k)
    int64_t* open_start;        // int64 [n]: rec_start of the burst still recording, or -1
    int32_t* open_nbytes;       // int32 [n]: its payload bytes committed so far
};
struct LiveStreamTapArgs {      // the tapped sink's kernel argument
    LiveStreamArgs s;
    LiveTapArgs t;
};
template <bool TAP>
struct LiveTapState {};
template <>
struct LiveTapState<true> {
    LiveTapArgs T;
    uint8_t* row;               // the channel's tap row
    int32_t n, mark;            // bytes committed in this push; n at the last report
};

template <bool TAP>
struct LiveStreamSinkT {
    using Args = std::conditional_t<TAP, LiveStreamTapArgs, LiveStreamArgs>;
    const LiveStreamArgs& A;
    int16_t* lwin;              // the wave's LDS window
    StreamDemod ds;
    int bf, lsh;
    uint32_t amp_thr;
    int16_t* gwin;              // the channel's window image
    uint8_t* pay;               // the channel's payload row
    LiveTapState<TAP> tp;

    static __device__ __forceinline__ const LiveStreamArgs& stream(const Args& a) {
        if constexpr (TAP) return a.s;
        else return a;
    }
    static __device__ __forceinline__ const LiveArgs& gate(const Args& a) { return stream(a).g; }
    // the block's four windows are the sink's own LDS; a wave takes its part
    __device__ __forceinline__ explicit LiveStreamSinkT(const Args& a) : A(stream(a)) {
        __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
        lwin = reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds);
        if constexpr (TAP) tp.T = a.t;
    }
    // what depends on the burst's rate (b = 0: no rate yet, nothing divides by it)
    __device__ __forceinline__ void set_rate(int b, int32_t amp_end) {
        bf = b;
        int l = 0;
        while ((2 << l) * 32 <= bf) l++;                         // lps = largest power of two <= bf / 32
        lsh = l;
        amp_thr = split_amp_thr(amp_end, bf);
    }
    // amp_end: the channel's squelch threshold (the per-symbol squelch of ref:375)
    __device__ __forceinline__ void init(const LiveArgs&, int c, int32_t amp_end) {
        ds = A.dm[c];
        set_rate(A.bit_frames[c], amp_end);
        rows(c);
    }
    // the channel's window image, payload row and tap row
    __device__ __forceinline__ void rows(int c) {
        gwin = A.win + (int64_t)c * kStreamWin;
        pay = A.pay + (int64_t)c * A.max_payload;
        if constexpr (TAP) {
            tp.row = tp.T.bytes + (int64_t)c * tp.T.cap;
            tp.n = 0;
            tp.mark = 0;
        }
    }
    // samples [from, to) of the open burst (positions in the burst) between the window image and the LDS window
    __device__ __forceinline__ void copy_tail(bool out, int64_t from, int64_t to, int lane) {
        for (int64_t p = from + lane; p < to; p += 64) {
            const int i = (int)(p & (kStreamWin - 1));
            if (out) gwin[i] = lwin[i];
            else lwin[i] = gwin[i];
        }
    }
    __device__ __forceinline__ bool live_demod(const LiveChan& st) const {
        return st.mode == 2 && ds.phase < 3 && st.rec_len <= kMaxStreamLen;
    }
    __device__ __forceinline__ int64_t tail_from(const LiveChan& st) const {
        return ds.phase == 0 ? 0 : (int64_t)ds.ci + (int64_t)ds.k * bf;
    }
    __device__ __forceinline__ void begin(const LiveArgs&, int lane, const LiveChan& st) {
        if (live_demod(st)) copy_tail(false, tail_from(st), st.rec_len, lane);
        wave_lds_sync();
    }
    __device__ __forceinline__ bool overflowed(const LiveArgs&, const LiveChan& st) const {
        return st.rec_len > kMaxStreamLen;
    }
    __device__ __forceinline__ void slot(const LiveArgs&, int64_t, int, const LiveChan&, bool) const {}
    // the burst's DemodOutputs, as afsk_demod_batch_uniform answers its recorded samples
    __device__ __forceinline__ void report(const LiveArgs&, int64_t i, const LiveChan& st, bool ovf, int32_t, int lane) {
        int32_t status, nbits = 0, ci = -1, term = -1, corrected = 0;
        if (ovf) status = AFSK_ST_BAD_LENGTH;
        else if (ds.phase == 0) status = AFSK_ST_TOO_SHORT;       // fewer than 4096 samples (ref:323-325)
        else {
            ci = ds.ci;
            if (ds.phase == 1) term = ds.ci + ds.k * bf;          // no terminator: after the last symbol
            else {
                term = ds.ci + ds.first * bf;                     // ref:368
                nbits = ds.nbits;
                corrected = ds.corrected;
            }
            status = nbits == 0 ? AFSK_ST_NO_DATA : AFSK_ST_OK;   // ref:422-424
        }
        const int32_t nbytes = (nbits / 7) >> 1;
        if (lane == 0) {
            A.out_nbytes[i] = nbytes;
            A.out_nbits[i] = nbits;
            A.out_clock_idx[i] = ci;
            A.out_term_frame[i] = term;
            A.out_status[i] = status;
            if (A.out_corrected) A.out_corrected[i] = corrected;
        }
        int32_t nb = nbytes < A.max_payload ? nbytes : A.max_payload;
        nb = nb < A.out_stride ? nb : A.out_stride;
        if (nb > 0) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");    // lane 0's payload stores, visible to the wave
            uint8_t* row = A.out_bytes + i * A.out_stride;
            for (int b = lane; b < nb; b += 64) row[b] = pay[b];
        }
        if constexpr (TAP) {
            if (ovf) tp.n = tp.mark;                              // not decoded: this push's bytes of it are withdrawn
            if (lane == 0) tp.T.len[i] = tp.n - tp.mark;
            tp.mark = tp.n;
        }
    }
    __device__ __forceinline__ void start(const LiveChan&) { ds = StreamDemod{}; }

    // data symbols of one 32-symbol word: decisions d, loud flags l (bit i = symbol k0 + i), m of them
    __device__ __forceinline__ void step(uint32_t d, uint32_t l, int m, int32_t k0, int lane) {
        int s = 0;
        if (ds.phase == 1) {
            // terminator: first k with decisions (k-3 .. k) = 1,0,0,0 (ref:361-366, 386-390)
            const uint64_t ext = ((uint64_t)d << 3) | (ds.bits & 7u);
            const uint64_t hit = ext & ~(ext >> 1) & ~(ext >> 2) & ~(ext >> 3) & ((1ull << m) - 1ull);
            if (!hit) {
                ds.bits = (uint32_t)(ext >> m) & 7u;
                return;
            }
            const int t = __builtin_ctzll(hit);
            ds.first = k0 + t + 1;
            ds.phase = 2;
            ds.bits = 0;
            s = t + 1;
        }
        const int r = m - s;
        if (r <= 0) return;
        const uint32_t mask = r >= 32 ? ~0u : ((1u << r) - 1u);
        const uint32_t quiet = ~(l >> s) & mask;                   // squelch stop (ref:372-376)
        int take = r;
        if (quiet) {
            take = __builtin_ctz(quiet);
            ds.phase = 3;
        }
        if (take == 0) return;
        const uint32_t tmask = take >= 32 ? ~0u : ((1u << take) - 1u);
        int have = ds.nbits % 7;
        int32_t cw_index = ds.nbits / 7;
        uint64_t acc = (uint64_t)(ds.bits & 0x7Fu) | ((uint64_t)((d >> s) & tmask) << have);
        uint32_t hi = (ds.bits >> 8) & 0xFu;
        ds.nbits += take;
        have += take;
        // ECC.decode (ref:154-163) + __bitsToBytes (ref:393-399): byte b = codewords 2b, 2b + 1
        while (have >= 7) {
            const uint32_t cw = (uint32_t)acc & 0x7Fu;
            acc >>= 7;
            have -= 7;
            ds.corrected += hamming_syndrome(cw) != 0u;
            const uint32_t nib = hamming_nibble(cw);
            if (cw_index & 1) {
                const int32_t b = cw_index >> 1;
                if (b < A.max_payload && lane == 0) pay[b] = (uint8_t)((hi << 4) | nib);
                if constexpr (TAP) {                              // (never past the row, whatever the input)
                    if (tp.n < tp.T.cap && lane == 0) tp.row[tp.n] = (uint8_t)((hi << 4) | nib);
                    tp.n++;
                }
            } else {
                hi = nib;
            }
            cw_index++;
        }
        ds.bits = ((uint32_t)acc & 0x7Fu) | (hi << 8);
    }

    // the block into the window; false: nothing to demodulate (stopped, too long to decode, or the burst's first block)
    __device__ __forceinline__ bool put(const LiveChan& st, const vec16 (&cur)[4], int lane) {
        if (!live_demod(st) || st.rec_len + kListenBlock > kMaxStreamLen) return false;   // stopped, or too long to decode
        const int32_t jb = (int32_t)(st.rec_len >> 11);           // the block's index in the burst
        uint8_t* half = reinterpret_cast<uint8_t*>(lwin) + (jb & 1) * (2 * kListenBlock);
        wave_lds_sync();                                           // the previous block's reads are done
#pragma unroll
        for (int j = 0; j < 4; j++) *reinterpret_cast<vec16*>(half + 1024 * j + 16 * lane) = cur[j];
        wave_lds_sync();
        return jb != 0;
    }
    // the clock index at bit_frames b of the burst's first 4096 samples, which the window holds (ref:322-339)
    __device__ __forceinline__ int clock(int b, int lane) const {
        FastRing fr;
        fr.ring = reinterpret_cast<uint8_t*>(lwin);
        fr.lane = lane;
        fr.next = 8;
        fr.warm_ops = 0;
        if (b == 40) {
            if (clock_index_is_zero<40, 8>(fr)) return 0;          // ref:332-337 (no search needed)
            return recover_clock_index_lanes<40, false, 8>(fr);
        }
        return recover_clock_index_rt(fr, b);
    }
    // the terminator search starts at symbol 0 of clock index ci
    __device__ __forceinline__ void lock(int ci) {
        ds.ci = ci;
        ds.k = 0;
        ds.phase = 1;
        ds.bits = 0;
        wave_lds_sync();
    }
    // the symbols that are complete with the block after st.rec_len and not committed yet
    __device__ __forceinline__ void symbols(const LiveChan& st, int lane) {
        const int32_t len = (int32_t)st.rec_len + kListenBlock;
        const int32_t k_end = (len - ds.ci - 1) / bf;             // symbols with i < len - bf (ref:362, 372)
        const int spp = 64 >> lsh;
        while (ds.k < k_end && ds.phase < 3) {
            const int n = k_end - ds.k < spp ? k_end - ds.k : spp;
            uint64_t dec, loud;
            stream_symbols(lwin, lane, bf, lsh, ds.ci + ds.k * bf, n, amp_thr, dec, loud);
            for (int h = 0; h < n && ds.phase < 3; h += 32) {
                const int m = n - h < 32 ? n - h : 32;
                step((uint32_t)(dec >> h), (uint32_t)(loud >> h), m, ds.k + h, lane);
            }
            ds.k += n;
        }
    }
    __device__ __forceinline__ void record(const LiveArgs&, const LiveChan& st, const vec16 (&cur)[4], int lane) {
        if (!put(st, cur, lane)) return;
        if (ds.phase == 0) lock(clock(bf, lane));                  // the first 4096 samples: clock recovery
        symbols(st, lane);
    }
    __device__ __forceinline__ int32_t head(const LiveChan&) const { return 0; }
    // what the next push needs of the open burst leaves the window; the demodulator state is stored
    __device__ __forceinline__ void finish(const LiveArgs&, int c, const LiveChan& st, int lane) {
        wave_lds_sync();
        if (live_demod(st)) copy_tail(true, tail_from(st), st.rec_len, lane);
        if (lane == 0) A.dm[c] = ds;
        if constexpr (TAP) {
            if (lane == 0) {
                const bool open = st.mode == 2;                     // (a flush has reported it: nothing is open)
                tp.T.n[c] = tp.n;
                tp.T.open_start[c] = open ? st.rec_start : -1;
                tp.T.open_nbytes[c] = open && ds.phase >= 2 ? (ds.nbits / 7) >> 1 : 0;
            }
        }
    }
    __device__ __forceinline__ void clear(const LiveArgs&, int64_t slot0, int i) const {
        const int64_t s = slot0 + i;
        A.out_nbytes[s] = 0;
        A.out_nbits[s] = 0;
        A.out_clock_idx[s] = -1;
        A.out_term_frame[s] = -1;
        A.out_status[s] = AFSK_ST_TOO_SHORT;
        if (A.out_corrected) A.out_corrected[s] = 0;
        if constexpr (TAP) tp.T.len[s] = 0;
    }
};
using LiveStreamSink = LiveStreamSinkT<false>;

__global__ __launch_bounds__(256) void live_stream_reset_kernel(LiveChan* chan, StreamDemod* dm, const uint8_t* mask,
                                                                int32_t n) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n && (!mask || mask[c])) {
        chan[c] = LiveChan{};
        dm[c] = StreamDemod{};
    }
}

}  // namespace afsk

namespace afsk {

int live_stream_reset(afsk_live* live, const uint8_t* d_mask_or_null, hipStream_t stream) {
    const LiveStreamLayout& L = live->SL;
    uint8_t* d = live->state.ptr();
    hipLaunchKernelGGL(live_stream_reset_kernel, dim3((uint32_t)((L.n + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<LiveChan*>(d), reinterpret_cast<StreamDemod*>(d + L.o_demod), d_mask_or_null,
                       (int32_t)L.n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch live_stream_reset_kernel");
}

// the streaming receiver's part of live_create (afsk_live.hip): the layout, the host fields that depend on it, the state
int live_stream_state(const LiveSpec& sp, afsk_live& lv) {
    LiveStreamLayout& L = lv.SL;
    if (int rc = live_stream_layout(sp.n_channels, sp.max_payload_len, sp.max_chunk_len, L, sp.per_channel)) return rc;
    lv.L.n = L.n;
    lv.L.slots = L.slots;
    lv.bit_frames = 0;
    lv.max_payload_len = sp.max_payload_len;
    // the channel states, carries (never read before written) and demodulators zeroed, the rates (and the channels'
    // thresholds behind them) uploaded
    std::vector<int32_t> up(sp.bit_frames, sp.bit_frames + L.n);
    if (sp.per_channel) {
        lv.o_thr = L.o_bf + 4 * L.n;
        up.insert(up.end(), sp.amp_start, sp.amp_start + L.n);
        up.insert(up.end(), sp.amp_end, sp.amp_end + L.n);
    }
    return lv.state.create(sp.entry, L.bytes, L.o_bf, up.data(), L.o_bf, 4 * (int64_t)up.size());
}

}  // namespace afsk

extern "C" {

int afsk_live_stream_layout(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len, int32_t* out_slots,
                            int64_t* out_state_bytes) {
    afsk::LiveStreamLayout L;
    if (int rc = afsk::live_stream_layout(n_channels, max_payload_len, max_chunk_len, L)) return rc;
    if (out_slots) *out_slots = (int32_t)L.slots;
    if (out_state_bytes) *out_state_bytes = L.bytes;
    return AFSK_OK;
}

int afsk_live_create_stream(int32_t n_channels, const int32_t* bit_frames_host, int32_t amp_start_threshold,
                            int32_t amp_end_threshold, int32_t max_payload_len, int32_t max_chunk_len, afsk_live** out) {
    bool same;
    if (int rc = live_check_rates(n_channels, bit_frames_host, out, same)) return rc;
    return live_create({"afsk_live_create_stream", n_channels, bit_frames_host, true, &amp_start_threshold,
                        &amp_end_threshold, false, true, 0, max_payload_len, max_chunk_len}, out);
}

int afsk_live_create_stream_thresholds(int32_t n_channels, const int32_t* bit_frames_host, const int32_t* amp_start_host,
                                       const int32_t* amp_end_host, int32_t max_payload_len, int32_t max_chunk_len,
                                       afsk_live** out) {
    bool same;
    if (int rc = live_check_rates(n_channels, bit_frames_host, out, same)) return rc;
    if (!amp_start_host || !amp_end_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    // one pair for every channel: the receiver afsk_live_create_stream builds
    const bool per_channel = !all_equal(amp_start_host, n_channels) || !all_equal(amp_end_host, n_channels);
    return live_create({"afsk_live_create_stream_thresholds", n_channels, bit_frames_host, true, amp_start_host,
                        amp_end_host, per_channel, true, 0, max_payload_len, max_chunk_len}, out);
}

}  // extern "C"
