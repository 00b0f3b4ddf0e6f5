// afsk_live_auto.hip -- the auto-rate streaming live receiver (afsk_live_create_stream_auto / afsk_live_push_auto,
// include/afsk_amd.h): the streaming receiver (afsk_live_stream.hip) with every BURST's rate decided on the device, from
// the burst's first 4096 samples, at the moment its second block is recorded -- the point where the fixed-rate sink runs
// clock recovery for the channel's rate.  From there on the burst is what the fixed-rate sink makes of it at the
// winner's rate: the sink's own code, with bf, lsh and amp_thr per burst instead of per channel.
//
// The decision is afsk_detect_rate_batch's (afsk_detect.hip), candidate by candidate on the wave's LDS window:
//   ci     the clock search the fixed-rate sink runs (LiveStreamSinkT::clock): by definition the detector's clock index
//   score  ONE pass over window samples [ci, ci + n 2bf), n = (4096 - 2bf - 1 - ci) / (2bf) + 1 whole cycles:
//            sum_k total(ci + k 2bf) = 65535 bf n - sum_p s(p) x[p],   s(p) = +1 where the training cycle is high at phase
//            (p - ci) mod 2bf (quarters 0 and 2 of the mark symbol, the first half of the space symbol), else -1
//          a lane takes every 64th sample and steps its phase by 64 mod 2bf (no division per sample); a wave sum, one
//          division per candidate.  |sum| < 2^27, 65535 bf n <= 2^27.
//   winner the minimum of (score << 6) | list position: the smallest score, the earliest candidate on a tie
// No LDS beyond the window (the detector's prefix-sum form would take 16 KiB more per wave), no scratch.
//
// The open burst's rate and score live in StreamDemod::spare -- (score << 11) | bit_frames, bit_frames <= 2044 < 2^11,
// score < 2^16 -- so they survive across pushes and are cleared wherever StreamDemod is: start, reset, masked reset,
// and the burst after a flush.  0 = no rate yet (fewer than 4096 samples).  A burst whose best score exceeds max_score
// (>= 0) is stopped where it would lock: phase 3, bit_frames 0, the score kept; it reports AFSK_ST_INVALID_BAUD.
//
// LiveAutoSinkT<TAP> derives from LiveStreamSinkT<TAP> and replaces init, record, report and clear; everything else --
// the window, the symbols, the terminator search, the squelch stop, Hamming, the payload row, the tap -- is the base's.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), after
// afsk_live_tap.hip and before afsk_live_push.hip.

namespace afsk {

constexpr int kLiveAutoMaxCand = AFSK_DETECT_MAX_CANDIDATES;
constexpr int kLiveAutoRateBits = 11;
static_assert(AFSK_SYNC_WINDOW / 2 <= (1 << kLiveAutoRateBits), "a valid bit_frames fits the rate bits of StreamDemod::spare");

// the auto part of an auto cell's kernel argument: by value, as the detector's candidate list
struct LiveAutoDetect {
    int32_t* out_bit_frames;            // int32 [n, slots]
    int32_t* out_rate_score;            // int32 [n, slots]
    int32_t max_score;                  // < 0: none
    int32_t n_cand;
    int32_t cand[kLiveAutoMaxCand];
};
template <bool TAP>
struct LiveAutoArgsT {
    typename LiveStreamSinkT<TAP>::Args b;      // the streaming sink's argument (with the tap's when TAP)
    LiveAutoDetect d;
};

template <bool TAP>
struct LiveAutoSinkT : LiveStreamSinkT<TAP> {
    using Base = LiveStreamSinkT<TAP>;
    using Args = LiveAutoArgsT<TAP>;
    using Base::A;
    using Base::bf;
    using Base::ds;
    using Base::lwin;
    const LiveAutoDetect& D;
    int32_t amp_end;                    // the channel's squelch threshold, for the rate a burst turns out to have

    static __device__ __forceinline__ const LiveArgs& gate(const Args& a) { return Base::gate(a.b); }
    __device__ __forceinline__ explicit LiveAutoSinkT(const Args& a) : Base(a.b), D(a.d) {}

    __device__ __forceinline__ int32_t rate() const { return ds.spare & ((1 << kLiveAutoRateBits) - 1); }
    __device__ __forceinline__ int32_t score() const { return ds.spare >> kLiveAutoRateBits; }
    __device__ __forceinline__ bool rejected() const { return ds.phase == 3 && rate() == 0; }

    // an open burst's rate comes back with its demodulator (0 while it has none)
    __device__ __forceinline__ void init(const LiveArgs&, int c, int32_t amp_end_) {
        ds = A.dm[c];
        amp_end = amp_end_;
        Base::set_rate(rate(), amp_end);
        Base::rows(c);
    }

    // the score of candidate b at clock index ci over the window (see the head of the file)
    __device__ __forceinline__ int32_t rate_score(int b, int ci, int lane) const {
        const int W = 2 * b, q = b >> 2;
        const int n = (kStreamWin - W - 1 - ci) / W + 1;
        const int total = n * W;                                   // ci + total <= 4095
        const int inc = 64 % W;
        int ph = lane % W;
        int32_t acc = 0;
        for (int j = lane; j < total; j += 64) {
            const int32_t x = lwin[ci + j];
            const bool high = ph < q || (ph >= 2 * q && ph < 3 * q) || (ph >= b && ph < b + 2 * q);
            acc += high ? x : -x;
            ph += inc;
            if (ph >= W) ph -= W;
        }
        const int32_t sum = __builtin_amdgcn_readlane(wave_incl_scan_dpp(acc), 63);
        return (int32_t)((65535u * (uint32_t)(b * n) - (uint32_t)sum) / (uint32_t)total);
    }

    // the burst's first 4096 samples are in the window: its rate, and the demodulator locked to it (or stopped)
    __device__ __forceinline__ void decide(int lane) {
        uint32_t best = 0xffffffffu;
        int best_ci = 0;
        for (int p = 0; p < D.n_cand; p++) {
            const int b = D.cand[p];
            const int ci = __builtin_amdgcn_readfirstlane(Base::clock(b, lane));
            const uint32_t key = ((uint32_t)rate_score(b, ci, lane) << 6) | (uint32_t)p;
            if (key < best) {
                best = key;
                best_ci = ci;
            }
        }
        const int32_t sc = (int32_t)(best >> 6);
        if (D.max_score >= 0 && sc > D.max_score) {
            ds.spare = sc << kLiveAutoRateBits;
            ds.phase = 3;
            return;
        }
        const int b = D.cand[best & 63u];
        ds.spare = (sc << kLiveAutoRateBits) | b;
        Base::set_rate(b, amp_end);
        Base::lock(best_ci);
    }

    __device__ __forceinline__ void record(const LiveArgs&, const LiveChan& st, const vec16 (&cur)[4], int lane) {
        if (!Base::put(st, cur, lane)) return;
        if (ds.phase == 0) decide(lane);
        if (ds.phase < 3) Base::symbols(st, lane);
    }

    __device__ __forceinline__ void report(const LiveArgs& g, int64_t i, const LiveChan& st, bool ovf, int32_t flags,
                                           int lane) {
        Base::report(g, i, st, ovf, flags, lane);
        if (lane == 0) {
            const bool rated = ds.phase != 0;                      // it reached 4096 samples
            D.out_bit_frames[i] = rated ? rate() : 0;
            D.out_rate_score[i] = rated ? score() : -1;
            if (!ovf && rejected()) {                              // not demodulated: no clock index, no bits
                A.out_clock_idx[i] = -1;
                A.out_term_frame[i] = -1;
                A.out_status[i] = AFSK_ST_INVALID_BAUD;
            }
        }
    }

    __device__ __forceinline__ void clear(const LiveArgs& g, int64_t slot0, int i) const {
        Base::clear(g, slot0, i);
        D.out_bit_frames[slot0 + i] = 0;
        D.out_rate_score[slot0 + i] = -1;
    }
};

}  // namespace afsk

extern "C" {

int afsk_live_create_stream_auto(int32_t n_channels, const int32_t* cand_bit_frames_host, int32_t n_cand,
                                 int32_t max_score, const int32_t* amp_start_host, const int32_t* amp_end_host,
                                 int32_t max_payload_len, int32_t max_chunk_len, int32_t tap, afsk_live** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (n_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (n_cand < 1 || n_cand > afsk::kLiveAutoMaxCand)
        return afsk::fail(AFSK_E_INVALID_ARG, "n_cand must be 1 ... AFSK_DETECT_MAX_CANDIDATES");
    if (tap != 0 && tap != 1) return afsk::fail(AFSK_E_INVALID_ARG, "tap must be 0 or 1");
    if (!cand_bit_frames_host || !amp_start_host || !amp_end_host)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t k = 0; k < n_cand; k++)
        if (!afsk::bf_valid(cand_bit_frames_host[k])) return afsk::fail_bit_frames();
    int32_t cap = 0;
    if (tap)                // the tap row is sized by the smallest candidate: no burst commits more bytes in a push
        if (int rc = afsk::live_tap_cap(n_channels, max_payload_len, max_chunk_len,
                                        *std::min_element(cand_bit_frames_host, cand_bit_frames_host + n_cand), cap))
            return rc;
    return afsk::no_throw([&] {
        // the streaming state; its bit_frames part stays 0: a channel has no rate of its own
        const std::vector<int32_t> none((size_t)n_channels, 0);
        const bool per_channel = !all_equal(amp_start_host, n_channels) || !all_equal(amp_end_host, n_channels);
        if (int rc = live_create({"afsk_live_create_stream_auto", n_channels, none.data(), true, amp_start_host,
                                  amp_end_host, per_channel, true, 0, max_payload_len, max_chunk_len}, out))
            return rc;
        afsk_live& lv = **out;
        lv.tap_cap = cap;
        lv.auto_n_cand = n_cand;
        lv.auto_max_score = max_score < 0 ? -1 : max_score;
        std::copy(cand_bit_frames_host, cand_bit_frames_host + n_cand, lv.auto_cand);
        return AFSK_OK;
    });
}

}  // extern "C"
