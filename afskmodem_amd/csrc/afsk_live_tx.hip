// afsk_live_tx.hip -- the live transmitter (afsk_live_tx_*, include/afsk_amd.h): Transmitter.transmit
// (afskmodem.py:472-478) for many channels played out chunk by chunk, each channel with a device-resident queue of
// messages that go out back to back.
//
// A submit is two launches: live_tx_order_kernel (one block) finds the first message whose channel is below its
// predecessor's, then live_tx_submit_kernel walks every run of equal channels before it with one thread, in order:
// check, take a ring entry, assign the start, copy the payload.  Nothing but the array order decides the queue order.
//
// A pull is two launches, in order on the caller's stream (a captured graph of them is a linear chain):
//   live_tx_tile_kernel   one wave per (channel, 1, 2 or 4 consecutive tiles of kTxTile samples of the pull): loads
//                         the channel state and its descriptor ring at once (the ring into LDS when it fits), then per
//                         tile finds the message whose tones meet it and renders it with modulate_kernel_t's
//                         scheme (payload window, tone-kind ballot, quarter-symbol bitmap, tone_words), 8 samples per
//                         16-byte store; reads the channel state, writes only the caller's buffer
//   live_tx_commit_kernel one thread per channel: advances pos, retires the messages that have ended, writes pending
//
// A ragged pull (afsk_live_tx_pull_ragged) is the same two launches in their RAGGED form: channel c renders and advances
// by len_c = clamp(lens[c], 0, T) samples, lens a DEVICE int32 [n] array read by the kernels.  A block renders tiles of
// one channel, so len_c is one block-uniform scalar load; tiles at or past len_c do nothing, the tile that straddles
// it is cut there (tx_store's partial store), and columns [len_c, T) of the row are not written.
//
// A hold pull (afsk_live_tx_pull_hold) is the ragged pull with carrier sense, again two launches: a channel whose
// hold[c] is set starts no message in this pull, and after a hold none starts for `holdoff` further samples (the wait
// counter w in TxChan::pad[0]).  live_tx_tile_hold_kernel renders the messages that have not begun `delta` samples
// later (tx_hold_delta) without writing state; live_tx_commit_hold_kernel derives the same delta, writes the shifted
// starts into the ring, the channel's end, w and deferred[c], and then commits as the other pulls do.
//
// A csma pull (afsk_live_tx_pull_csma) is the hold pull with p-persistence: the same tile launch (it only reads w), and
// live_tx_commit_csma_kernel in place of the hold commit -- a held channel's wait becomes holdoff + slot * G with G drawn
// from a counter hash (the draw counter k in TxChan::pad[1]), and on_air[c] reports the columns of the pull that carry
// the channel's tones.
//
// A mixed transmitter (afsk_live_tx_create_mixed) keeps each channel's bit_frames and training symbols in a TxGeom
// array past the uniform layout; submit and live_tx_tile_kernel_mixed read them per channel, and the tile kernel picks
// the small- or large-q tone code per wave (a wave renders tiles of one channel, so the branch is wave-uniform).
//
// A rated transmitter (afsk_live_tx_create_rated) keeps a table of up to AFSK_DETECT_MAX_CANDIDATES geometries and one
// TxGeom per RING ENTRY past the uniform layout: a submit (afsk_live_tx_submit_rated, or the relay's
// afsk_live_tx_submit_events_rated) writes the message's geometry next to its descriptor, and
// live_tx_tile_kernel_rated loads the channel's geometry ring with its descriptor ring and renders every tile with the
// geometry of the message the tile meets (the tone code again chosen per wave and tile).
//
// Every message is at least 4 symbols + the 4800-sample silent tail long, so the tones of two messages of a channel
// are at least 4800 samples apart and a tile of at most 4096 samples meets the tones of one message at most.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end): it uses that
// file's store16, hamming_codeword / symbol_is_mark, q_words, kWinBytes and tone_words.
#include <memory>
#include <new>
#include <vector>

#include "../../include/afsk_amd.h"
#include "afsk_capi_internal.h"

namespace afsk {

struct TxChan {             // 32 bytes per channel
    int64_t pos;            // samples of the current stream pulled so far
    int64_t end;            // end (stream index) of the last message queued; <= pos once the queue has drained
    int32_t head;           // ring entry of the oldest message not yet fully emitted
    int32_t count;          // messages queued or on air
    int32_t pad[2];         // pad[0]: the hold pull's wait counter w (afsk_live_tx_pull_hold; 0 after create and reset,
                            // neither read nor written by the plain and ragged pulls); pad[1]: the csma pull's draw
                            // counter k (afsk_live_tx_pull_csma; 0 after create and reset, touched by no other pull)
};
static_assert(sizeof(TxChan) == 32, "TxChan layout");

struct TxDesc {             // 16 bytes per ring entry
    int64_t start;          // stream index of the first sample
    int32_t n_samples;      // .wav samples of the message: tones + 4800 silent samples
    int32_t payload_len;
};
static_assert(sizeof(TxDesc) == 16, "TxDesc layout");

struct TxGeom {             // 8 bytes per channel of a mixed transmitter, per table and ring entry of a rated one
    int32_t bf;             // bit_frames: a multiple of 4 in 4 ... 48000
    int32_t n_train_sym;    // 2 * ts_cycles (ts_cycles >= 0)
};
static_assert(sizeof(TxGeom) == 8, "TxGeom layout");

constexpr int kTxThreads = 64;                                  // one wave per block
constexpr int kTxIters = 8;                                     // 16-byte stores per lane and tile
constexpr int kTxTile = kTxThreads * 8 * kTxIters;              // samples per tile
static_assert(kTxTile < AFSK_TAIL_SILENCE, "a tile must not meet the tones of two messages");
static_assert(kTxTile / 56 + 4 <= kWinBytes, "payload window too small for the tile");
constexpr int kTxLdsRing = 64;                                  // rings up to this depth are read from LDS
constexpr int kTxMinBlocks = 8192;                              // 32 waves per CU before tiles are shared
constexpr int kTxMaxDepth = 1024;
constexpr int kTxMaxPayload = 65536;

struct TxLayout {
    int64_t n = 0, depth = 0, max_payload = 0;
    int64_t o_desc = 0, o_slots = 0, o_scratch = 0, bytes = 0;
};

inline int64_t tx_align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// The state allocation: TxChan [n] | TxDesc [n, depth] | payload slots uint8 [n, depth, max_payload] | 256 bytes of
// submit scratch (the first unsorted message); every part 256-byte aligned.
inline int live_tx_layout(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len, TxLayout& L) {
    if (n_channels < 1) return fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (queue_depth < 1 || queue_depth > kTxMaxDepth)
        return fail(AFSK_E_INVALID_ARG, "queue_depth must lie in 1 ... 1024");
    if (max_payload_len < 0 || max_payload_len > kTxMaxPayload)
        return fail(AFSK_E_INVALID_ARG, "max_payload_len must lie in 0 ... 65536");
    if ((int64_t)n_channels * queue_depth > 0x7fffffffll)
        return fail(AFSK_E_INVALID_ARG, "n_channels * queue_depth exceeds 2^31 - 1");
    L.n = n_channels;
    L.depth = queue_depth;
    L.max_payload = max_payload_len;
    L.o_desc = tx_align256(32 * L.n);
    L.o_slots = L.o_desc + tx_align256(16 * L.n * L.depth);
    L.o_scratch = L.o_slots + tx_align256(L.n * L.depth * L.max_payload);
    L.bytes = L.o_scratch + 256;
    return AFSK_OK;
}

// A mixed transmitter's allocation: the uniform layout, then TxGeom [n] (256-byte aligned: L.bytes is).
inline int64_t live_tx_mixed_bytes(const TxLayout& L) { return L.bytes + tx_align256(8 * L.n); }

// A rated transmitter's allocation: the uniform layout, then the table TxGeom [n_rates], then TxGeom [n, depth] (one
// geometry per ring entry, written by the submit that writes the entry); each part 256-byte aligned.
struct TxRatedLayout {
    int64_t o_rates = 0, o_msg_geom = 0, bytes = 0;
};
inline TxRatedLayout live_tx_rated_layout(const TxLayout& L, int32_t n_rates) {
    TxRatedLayout R;
    R.o_rates = L.bytes;
    R.o_msg_geom = R.o_rates + tx_align256(8 * (int64_t)n_rates);
    R.bytes = R.o_msg_geom + tx_align256(8 * L.n * L.depth);
    return R;
}

// ------------------------------------------------------------------------------------------------------- submit

__global__ __launch_bounds__(256) void live_tx_order_kernel(const int32_t* channel, int32_t n, int32_t* first_bad) {
    __shared__ int32_t red[256];
    int32_t m = n;
    for (int32_t i = (int32_t)threadIdx.x + 1; i < n; i += 256)
        if (channel[i] < channel[i - 1]) { m = i; break; }      // a thread's indices rise: its first is its least
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *first_bad = red[0];
}

struct TxSubmitArgs {
    TxChan* chan;
    TxDesc* desc;
    uint8_t* slots;
    const int32_t* first_bad;
    const int32_t* channel;
    const int64_t* payload_offset;
    const int32_t* payload_len;
    const uint8_t* payload;
    const int32_t* out_index;   // NULL: outputs of message i at i
    int32_t* out_status;
    int64_t* out_start;
    int32_t* out_n_samples;
    int32_t n_msgs;
    int32_t n;
    int32_t depth;
    int32_t max_payload;
    int32_t bf;
    int32_t n_train_sym;
    const TxGeom* geom;         // mixed: per-channel bf / n_train_sym (NULL: the two above)
};

__global__ __launch_bounds__(256) void live_tx_submit_kernel(TxSubmitArgs a) {
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.n_msgs) return;
    auto put = [&](int32_t j, int32_t status, int64_t start, int32_t ns) {
        const int32_t k = a.out_index ? a.out_index[j] : j;
        if ((uint32_t)k >= (uint32_t)a.n_msgs) return;          // (not a permutation: nothing written for it)
        a.out_status[k] = status;
        a.out_start[k] = start;
        a.out_n_samples[k] = ns;
    };
    const int32_t first_bad = *a.first_bad;
    if (i >= first_bad) { put(i, AFSK_LIVE_TX_UNSORTED, -1, 0); return; }
    const int32_t ch = a.channel[i];
    if (i > 0 && a.channel[i - 1] == ch) return;                // not the first of its run
    const bool ok = ch >= 0 && ch < a.n;
    TxChan st = ok ? a.chan[ch] : TxChan{};
    const TxGeom g = ok && a.geom ? a.geom[ch] : TxGeom{a.bf, a.n_train_sym};
    for (int32_t j = i; j < first_bad && a.channel[j] == ch; j++) {
        const int32_t plen = a.payload_len[j];
        if (!ok) { put(j, AFSK_LIVE_TX_BAD_CHANNEL, -1, 0); continue; }
        if (plen < 0 || plen > a.max_payload) { put(j, AFSK_LIVE_TX_TOO_LONG, -1, 0); continue; }
        if (st.count >= a.depth) { put(j, AFSK_LIVE_TX_QUEUE_FULL, -1, 0); continue; }
        const int64_t start = st.pos > st.end ? st.pos : st.end;
        const int32_t ns = g.bf * (g.n_train_sym + 4 + 14 * plen) + AFSK_TAIL_SILENCE;   // <= AFSK_MAX_STREAM_LEN
        int32_t slot = st.head + st.count;
        if (slot >= a.depth) slot -= a.depth;
        const int64_t e = (int64_t)ch * a.depth + slot;
        a.desc[e] = TxDesc{start, ns, plen};
        uint8_t* dst = a.slots + e * a.max_payload;
        const uint8_t* src = a.payload + a.payload_offset[j];
        for (int32_t b = 0; b < plen; b++) dst[b] = src[b];
        st.end = start + ns;
        st.count++;
        put(j, AFSK_LIVE_TX_QUEUED, start, ns);
    }
    if (ok) a.chan[ch] = st;
}

// live_tx_submit_kernel for a rated transmitter (kept a kernel of its own: the one above is the code it was): message
// j plays at rates[rate_index[j]] (a null rate_index: rates[0]), an index outside 0 ... n_rates - 1 is
// AFSK_LIVE_TX_BAD_RATE -- behind _TOO_LONG, in front of _QUEUE_FULL -- and the geometry of a queued message goes to
// msg_geom next to its descriptor.
__global__ __launch_bounds__(256) void live_tx_submit_rated_kernel(TxSubmitArgs a, const int32_t* rate_index,
                                                                   const TxGeom* rates, int32_t n_rates,
                                                                   TxGeom* msg_geom) {
    const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (i >= a.n_msgs) return;
    auto put = [&](int32_t j, int32_t status, int64_t start, int32_t ns) {
        const int32_t k = a.out_index ? a.out_index[j] : j;
        if ((uint32_t)k >= (uint32_t)a.n_msgs) return;          // (not a permutation: nothing written for it)
        a.out_status[k] = status;
        a.out_start[k] = start;
        a.out_n_samples[k] = ns;
    };
    const int32_t first_bad = *a.first_bad;
    if (i >= first_bad) { put(i, AFSK_LIVE_TX_UNSORTED, -1, 0); return; }
    const int32_t ch = a.channel[i];
    if (i > 0 && a.channel[i - 1] == ch) return;                // not the first of its run
    const bool ok = ch >= 0 && ch < a.n;
    TxChan st = ok ? a.chan[ch] : TxChan{};
    for (int32_t j = i; j < first_bad && a.channel[j] == ch; j++) {
        const int32_t plen = a.payload_len[j];
        if (!ok) { put(j, AFSK_LIVE_TX_BAD_CHANNEL, -1, 0); continue; }
        if (plen < 0 || plen > a.max_payload) { put(j, AFSK_LIVE_TX_TOO_LONG, -1, 0); continue; }
        const int32_t r = rate_index ? rate_index[j] : 0;
        if (r < 0 || r >= n_rates) { put(j, AFSK_LIVE_TX_BAD_RATE, -1, 0); continue; }
        const TxGeom g = rates[r];
        if (st.count >= a.depth) { put(j, AFSK_LIVE_TX_QUEUE_FULL, -1, 0); continue; }
        const int64_t start = st.pos > st.end ? st.pos : st.end;
        const int32_t ns = g.bf * (g.n_train_sym + 4 + 14 * plen) + AFSK_TAIL_SILENCE;   // <= AFSK_MAX_STREAM_LEN
        int32_t slot = st.head + st.count;
        if (slot >= a.depth) slot -= a.depth;
        const int64_t e = (int64_t)ch * a.depth + slot;
        a.desc[e] = TxDesc{start, ns, plen};
        msg_geom[e] = g;
        uint8_t* dst = a.slots + e * a.max_payload;
        const uint8_t* src = a.payload + a.payload_offset[j];
        for (int32_t b = 0; b < plen; b++) dst[b] = src[b];
        st.end = start + ns;
        st.count++;
        put(j, AFSK_LIVE_TX_QUEUED, start, ns);
    }
    if (ok) a.chan[ch] = st;
}

// --------------------------------------------------------------------------------------------------------- pull

struct TxPullArgs {
    const TxChan* chan;
    const TxDesc* desc;
    const uint8_t* slots;
    int16_t* out;
    int64_t out_stride;
    int32_t T;
    int32_t tiles;              // tiles per channel: ceil(T / kTxTile)
    int32_t tiles_per_block;    // consecutive tiles of one channel a block renders
    int32_t blocks_per_row;     // ceil(tiles / tiles_per_block)
    int32_t depth;
    int32_t max_payload;
    uint32_t bf;
    uint32_t n_train_sym;
};

// The two samples of relative frame x (even): frame x's tone value twice (wav quirk ref:239-244).
__device__ __forceinline__ uint32_t tone_pair(uint32_t x, float rcp_q, const uint32_t* qb) {
    const uint32_t Q = (uint32_t)(((float)x + 0.5f) * rcp_q);
    return ((qb[Q >> 5] >> (Q & 31u)) & 1u) ? kHi2 : kLo2;
}

// Samples x .. x+7 of a message (x relative to its first sample, any sign and parity), zero outside its tones
// [0, lim).  xb: the relative frame of the first symbol in qb.  With the quirk, sample m is frame m & ~1, so an odd x
// takes the pairs of frames x-1 ... x+7 and shifts them by one sample.
template <bool SMALLQ>
__device__ __forceinline__ store16 msg_words(int32_t x, int32_t lim, int32_t xb, uint32_t q, float rcp_q,
                                             uint32_t mq, const uint32_t* qb, bool odd) {
    store16 w{0u, 0u, 0u, 0u};
    if (x + 8 <= 0 || x >= lim) return w;
    const int32_t xe = x & ~1;
    uint32_t p4 = 0u;                                                // the pair of frame xe + 8 (odd x only)
    if (xe >= 0 && xe + 10 <= lim) {
        w = tone_words<true, SMALLQ>((uint32_t)(xe - xb), q, rcp_q, mq, qb);
        if (odd) p4 = tone_pair((uint32_t)(xe + 8 - xb), rcp_q, qb);
    } else {                                                         // the message's first or last tone samples
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int32_t f = xe + 2 * d;
            w[d] = (f >= 0 && f < lim) ? tone_pair((uint32_t)(f - xb), rcp_q, qb) : 0u;
        }
        if (odd && xe + 8 < lim) p4 = tone_pair((uint32_t)(xe + 8 - xb), rcp_q, qb);
    }
    if (odd) {
        w[0] = __builtin_amdgcn_alignbit(w[1], w[0], 16);
        w[1] = __builtin_amdgcn_alignbit(w[2], w[1], 16);
        w[2] = __builtin_amdgcn_alignbit(w[3], w[2], 16);
        w[3] = __builtin_amdgcn_alignbit(p4, w[3], 16);
    }
    return w;
}

__device__ __forceinline__ void tx_store(int16_t* dst0, uint32_t j0, uint32_t len, store16 w) {
    int16_t* dst = dst0 + j0;
    if (j0 + 8u <= len) {
        *reinterpret_cast<store16*>(dst) = w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++)
            if (j0 + j < len) dst[j] = (int16_t)(w[j >> 1] >> (16u * (j & 1u)));
    }
}

// The tile's samples, 8 per lane and store (the message's tones from relative sample x0 on, zero past lim).
template <bool SMALLQ>
__device__ __forceinline__ void tx_render(int16_t* dst0, uint32_t len, int32_t x0, int32_t lim, int32_t xb, uint32_t q,
                                          float rcp_q, uint32_t mq, const uint32_t* qbits, bool odd) {
#pragma unroll 2
    for (int it = 0; it < kTxIters; it++) {
        const uint32_t j0 = ((uint32_t)it * kTxThreads + threadIdx.x) * 8u;
        if (j0 >= len) break;
        tx_store(dst0, j0, len, msg_words<SMALLQ>(x0 + (int32_t)j0, lim, xb, q, rcp_q, mq, qbits, odd));
    }
}

// The hold rule (afsk_live_tx_pull_hold, include/afsk_amd.h), shared by the tile kernels' hold form and the hold
// commit.  A channel that advances L samples in this pull lets no message begin before `earliest`: the end of the pull
// when it is held, else pos + w (w: the wait counter a hold left, TxChan::pad[0]).  u, the oldest message with
// start >= pos, and every message behind it move by delta = max(0, earliest - u.start).
__device__ __forceinline__ int64_t tx_hold_earliest(const TxChan& ch, int32_t L, bool held) {
    return ch.pos + (held ? L : ch.pad[0]);
}
__device__ __forceinline__ int64_t tx_hold_delta(int64_t earliest, int64_t u_start) {
    return earliest > u_start ? earliest - u_start : 0;
}

// The geometry ring of a rated transmitter's channel in LDS (KIND 3 alone: the other kinds have no such array).
template <int KIND>
__device__ __forceinline__ TxGeom* tx_geom_ring() {
    if constexpr (KIND == 3) {
        __shared__ TxGeom gring[kTxLdsRing];
        return gring;
    } else {
        return nullptr;
    }
}

// KIND 0 / 1: a uniform transmitter whose q = bf / 4 is >= 8 / < 8 (a.bf, a.n_train_sym); KIND 2: a mixed one, the
// channel's geometry from geom[c] and the tone code chosen per wave; KIND 3: a rated one, geom the per-entry
// geometries TxGeom [n, depth]: the geometry and the tone code are those of the message each tile meets, so nothing
// derived from them lives outside the tile loop.  RAGGED: the channel's samples end at
// clamp(lens[c], 0, a.T) instead of a.T (a null lens: a.T); the instantiations without the flag are the code they were.
// HOLD (afsk_live_tx_pull_hold): the channel's messages that have not begun (start >= pos) are rendered `delta` samples
// later, delta the hold rule's shift (tx_hold_delta) of the oldest of them, found in the tile's own ring walk -- one
// more block-uniform int32 load (hold[c]; the wait counter comes with the channel state).  The kernel only reads
// state: live_tx_commit_hold_kernel derives the same delta and writes the shifted starts.  The instantiations without
// the flag are the code they were.
template <int KIND, bool RAGGED = false, bool HOLD = false>
__device__ __forceinline__ void live_tx_tile(TxPullArgs a, const TxGeom* geom, const int32_t* lens = nullptr,
                                             const int32_t* hold = nullptr) {
    __shared__ uint8_t win[kWinBytes];
    __shared__ unsigned long long kinds[kTxTile / 4 / 64 + 2];
    __shared__ uint32_t qbits[q_words(kTxTile)];
    __shared__ TxDesc ring[kTxLdsRing];
    const int bid = xcd_block((int)blockIdx.x, (int)gridDim.x);
    const int c = bid / a.blocks_per_row;
    const int b = bid - c * a.blocks_per_row;
    uint32_t bf = a.bf;
    uint32_t n_train_sym = a.n_train_sym;
    uint32_t T = (uint32_t)a.T;                                        // samples of the channel in this pull
    if constexpr (RAGGED) {
        if (lens) {
            const int32_t l = lens[c];
            T = l < 0 ? 0u : min((uint32_t)l, T);
        }
        if ((uint32_t)(b * a.tiles_per_block) * kTxTile >= T) return;  // block-uniform: nothing of the channel here
    }
    // the channel state (and geometry) and its whole descriptor ring, loaded at once (no address depends on another
    // of these loads)
    const TxChan ch = a.chan[c];
    int64_t earliest = 0;                                              // HOLD: no message begins before this sample
    int64_t delta = -1;                                                // HOLD: the shift, < 0 until the walk meets u
    if constexpr (HOLD) earliest = tx_hold_earliest(ch, (int32_t)T, hold && hold[c] != 0);
    if (KIND == 2) {
        const TxGeom g = geom[c];
        bf = (uint32_t)g.bf;
        n_train_sym = (uint32_t)g.n_train_sym;
    }
    const TxDesc* gring = a.desc + (int64_t)c * a.depth;
    const uint8_t* gpay = a.slots + (int64_t)c * a.depth * a.max_payload;
    const bool lds_ring = a.depth <= kTxLdsRing;
    TxGeom* const lgeom = tx_geom_ring<KIND>();
    const TxGeom* ggeom = nullptr;                                     // KIND 3: the channel's geometry ring
    if constexpr (KIND == 3) ggeom = geom + (int64_t)c * a.depth;
    if (lds_ring && (int)threadIdx.x < a.depth) {
        ring[threadIdx.x] = gring[threadIdx.x];
        if constexpr (KIND == 3) lgeom[threadIdx.x] = ggeom[threadIdx.x];
    }
    __syncthreads();

    for (int k = 0; k < a.tiles_per_block; k++) {
        const int t = b * a.tiles_per_block + k;
        if (t >= a.tiles) break;                                       // block-uniform
        if (k > 0) __syncthreads();                                    // the previous tile's qbits / win are read
        const uint32_t t0 = (uint32_t)t * kTxTile;
        if constexpr (RAGGED) {
            if (t0 >= T) break;                                        // block-uniform
        }
        const uint32_t len = min((uint32_t)kTxTile, T - t0);          // samples of this tile
        int16_t* dst0 = a.out + (int64_t)c * a.out_stride + t0;
        const int64_t p0 = ch.pos + t0;

        // the message whose tones [start, start + n_samples - 4800) meet [p0, p0 + len): the ring is in stream order
        int64_t m0 = 0;                 // p0 relative to the message's first sample
        int32_t lim = 0;                // tone samples of the message (0: the tile is silent)
        uint32_t plen = 0;
        int32_t slot = 0;
        for (int32_t i = 0, e = ch.head; i < ch.count; i++, e = (e + 1 == a.depth ? 0 : e + 1)) {
            const TxDesc d = lds_ring ? ring[e] : gring[e];
            int64_t start = d.start;
            if constexpr (HOLD) {
                if (start >= ch.pos) {                                 // not begun: u (the first such) and all behind
                    if (delta < 0) delta = tx_hold_delta(earliest, start);
                    start += delta;
                }
            }
            if (start >= p0 + len) break;
            const int32_t tones = d.n_samples - AFSK_TAIL_SILENCE;
            if (start + tones > p0) {
                m0 = p0 - start;
                lim = tones;
                plen = (uint32_t)d.payload_len;
                slot = e;
                if constexpr (KIND == 3) {                             // the message's own geometry (wave-uniform)
                    const TxGeom g = lds_ring ? lgeom[e] : ggeom[e];
                    bf = (uint32_t)__builtin_amdgcn_readfirstlane(g.bf);
                    n_train_sym = (uint32_t)__builtin_amdgcn_readfirstlane(g.n_train_sym);
                }
                break;
            }
        }
        if (lim == 0) {
#pragma unroll
            for (int it = 0; it < kTxIters; it++) {
                const uint32_t j0 = ((uint32_t)it * kTxThreads + threadIdx.x) * 8u;
                if (j0 >= len) break;
                tx_store(dst0, j0, len, store16{0u, 0u, 0u, 0u});
            }
            continue;
        }

        // the tile meets the tones: m0 lies in (-len, lim)
        const int32_t x0 = (int32_t)m0;
        const uint32_t lo = x0 > 0 ? (uint32_t)x0 : 0u;
        const uint32_t Sb = lo / bf;                                   // first symbol the tile touches
        const uint32_t n_sym = n_train_sym + 4u + 14u * plen;
        const uint32_t data0 = n_train_sym + 4u;
        const uint32_t first_byte = ((Sb > data0 ? Sb - data0 : 0u) / 7u) >> 1;
        const uint32_t last = (lo + kTxTile + 15u) / bf + 2u;          // exclusive upper bound + slack (odd phase)
        const uint32_t nsym_blk = last - Sb + 1u;
        if (Sb + nsym_blk > data0) {                                   // block-uniform: data symbols
            // the bytes the tile's data symbols read: fewer than nsym_blk / 14 + 4 from first_byte
            const uint8_t* payload = gpay + (int64_t)slot * a.max_payload;
            const uint32_t need = min((uint32_t)kWinBytes, nsym_blk / 14u + 4u);
            for (uint32_t i = threadIdx.x; i < need; i += kTxThreads) {
                const uint32_t idx = first_byte + i;
                win[i] = idx < plen ? payload[idx] : (uint8_t)0;
            }
            __syncthreads();
        }
        {
            const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
            for (uint32_t r0 = wave * 64u; r0 < nsym_blk; r0 += kTxThreads) {
                const uint32_t S = Sb + r0 + lane;
                const bool mk = S < n_sym && symbol_is_mark(S, n_train_sym, first_byte, win);
                const unsigned long long m = __ballot(mk);
                if (lane == 0) kinds[r0 >> 6] = m;
            }
        }
        __syncthreads();
        {
            // quarter bitmap as modulate_kernel_t: word w = symbols Sb + 8w .. 8w+7, space 0b0011, mark 0b0101
            const uint32_t nwords = (nsym_blk + 7u) >> 3;
            for (uint32_t w = threadIdx.x; w <= nwords; w += kTxThreads) {
                uint32_t x = w < nwords ? (uint32_t)(kinds[w >> 3] >> ((w & 7u) * 8u)) & 0xFFu : 0u;
                x = (x | (x << 12)) & 0x000F000Fu;
                x = (x | (x << 6)) & 0x03030303u;
                x = (x | (x << 3)) & 0x11111111u;
                qbits[w] = 0x33333333u ^ (x * 6u);
            }
        }
        __syncthreads();
        const uint32_t q = bf >> 2;
        const float rcp_q = 1.0f / (float)q;
        const uint32_t mq = (65536u + q - 1u) / q;
        const int32_t xb = (int32_t)(Sb * bf);
        const bool odd = (x0 & 1) != 0;
        if (KIND >= 2) {                                               // block- (= wave-) uniform
            if (q < 8u) tx_render<true>(dst0, len, x0, lim, xb, q, rcp_q, mq, qbits, odd);
            else tx_render<false>(dst0, len, x0, lim, xb, q, rcp_q, mq, qbits, odd);
        } else {
            tx_render<KIND == 1>(dst0, len, x0, lim, xb, q, rcp_q, mq, qbits, odd);
        }
    }
}

template <bool SMALLQ>
__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_kernel(TxPullArgs a) {
    live_tx_tile<SMALLQ ? 1 : 0>(a, nullptr);
}

__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_kernel_mixed(
    TxPullArgs a, const TxGeom* geom) {
    live_tx_tile<2>(a, geom);
}

// A rated transmitter's tile kernel: msg_geom = TxGeom [n, depth], the geometry of every ring entry.
__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_kernel_rated(
    TxPullArgs a, const TxGeom* msg_geom) {
    live_tx_tile<3>(a, msg_geom);
}

// channel c advances by T samples: the messages that have ended are retired, pending is what is left
__device__ __forceinline__ void live_tx_commit(TxChan* chan, const TxDesc* desc, int c, int32_t depth, int32_t T,
                                               int32_t* pending) {
    TxChan st = chan[c];
    st.pos += T;
    while (st.count > 0) {
        const TxDesc d = desc[(int64_t)c * depth + st.head];
        if (d.start + d.n_samples > st.pos) break;
        st.head = st.head + 1 == depth ? 0 : st.head + 1;
        st.count--;
    }
    chan[c] = st;
    pending[c] = st.count;
}

__global__ __launch_bounds__(256) void live_tx_commit_kernel(TxChan* chan, const TxDesc* desc, int32_t n,
                                                             int32_t depth, int32_t T, int32_t* pending) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    live_tx_commit(chan, desc, c, depth, T, pending);
}

// The ragged pull's kernels (afsk_live_tx_pull_ragged): channel c ends at clamp(lens[c], 0, T), lens a DEVICE array.
template <bool SMALLQ>
__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_ragged_kernel(
    TxPullArgs a, const int32_t* lens) {
    live_tx_tile<SMALLQ ? 1 : 0, true>(a, nullptr, lens);
}

__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_ragged_kernel_mixed(
    TxPullArgs a, const TxGeom* geom, const int32_t* lens) {
    live_tx_tile<2, true>(a, geom, lens);
}

__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_ragged_kernel_rated(
    TxPullArgs a, const TxGeom* msg_geom, const int32_t* lens) {
    live_tx_tile<3, true>(a, msg_geom, lens);
}

__global__ __launch_bounds__(256) void live_tx_commit_ragged_kernel(TxChan* chan, const TxDesc* desc, int32_t n,
                                                                    int32_t depth, int32_t T, const int32_t* lens,
                                                                    int32_t* pending) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    if (lens) {
        const int32_t l = lens[c];
        T = l < 0 ? 0 : (l < T ? l : T);
    }
    live_tx_commit(chan, desc, c, depth, T, pending);
}

// The hold pull's kernels (afsk_live_tx_pull_hold): the ragged forms with the hold rule (lens and hold DEVICE arrays or
// NULL).
template <bool SMALLQ>
__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_hold_kernel(
    TxPullArgs a, const int32_t* lens, const int32_t* hold) {
    live_tx_tile<SMALLQ ? 1 : 0, true, true>(a, nullptr, lens, hold);
}

__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_hold_kernel_mixed(
    TxPullArgs a, const TxGeom* geom, const int32_t* lens, const int32_t* hold) {
    live_tx_tile<2, true, true>(a, geom, lens, hold);
}

__global__ __launch_bounds__(kTxThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void live_tx_tile_hold_kernel_rated(
    TxPullArgs a, const TxGeom* msg_geom, const int32_t* lens, const int32_t* hold) {
    live_tx_tile<3, true, true>(a, msg_geom, lens, hold);
}

// One thread per channel: the hold rule's writes, then live_tx_commit.  It derives the delta the tile kernel rendered
// with from the same state, adds it to the start of u and of every ring entry behind u (entries head + i ... head +
// count - 1, wrapping at depth; read from global memory whatever the depth) and to the channel's end, sets the wait
// counter (holdoff when held, else what is left of it after L samples) and writes deferred[c].
__global__ __launch_bounds__(256) void live_tx_commit_hold_kernel(TxChan* chan, TxDesc* desc, int32_t n, int32_t depth,
                                                                  int32_t T, const int32_t* lens, const int32_t* hold,
                                                                  int32_t holdoff, int32_t* pending,
                                                                  int64_t* deferred) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    if (lens) {
        const int32_t l = lens[c];
        T = l < 0 ? 0 : (l < T ? l : T);
    }
    TxChan st = chan[c];
    const bool held = hold && hold[c] != 0;
    const int64_t earliest = tx_hold_earliest(st, T, held);
    TxDesc* ring = desc + (int64_t)c * depth;
    int64_t delta = 0;
    for (int32_t i = 0, e = st.head; i < st.count; i++, e = (e + 1 == depth ? 0 : e + 1)) {
        if (delta == 0) {
            const int64_t start = ring[e].start;
            if (start < st.pos) continue;                              // on air, or in its silent tail
            delta = tx_hold_delta(earliest, start);                    // e is u
            if (delta == 0) break;
        }
        ring[e].start += delta;
    }
    st.end += delta;                                                   // (delta > 0: u is queued, so end >= u's end)
    const int32_t w = st.pad[0];
    st.pad[0] = held ? holdoff : (w > T ? w - T : 0);
    chan[c] = st;
    deferred[c] = delta;
    live_tx_commit(chan, desc, c, depth, T, pending);
}

// The csma pull's draw (afsk_live_tx_pull_csma): the slots a released channel waits past its holdoff, G = the first j in
// 0 ... 254 whose draw (hash32(base ^ j) & 255) is <= persist, 255 when there is none; base is keyed by the seed, the
// channel and the channel's draw counter k, so every held pull draws afresh and no two channels share a sequence.
__device__ __forceinline__ int32_t tx_csma_slots(uint32_t seed, int c, uint32_t k, int32_t persist) {
    const uint32_t base = hash32(hash32(seed ^ hash32((uint32_t)c + 0x9e3779b9U)) ^ k);
    int32_t g = 0;
    while (g < 255 && (int32_t)(hash32(base ^ (uint32_t)g) & 255u) > persist) g++;
    return g;
}

// live_tx_commit_hold_kernel with p-persistence (afsk_live_tx_pull_csma): a held channel's wait becomes holdoff + slot * G
// (tx_csma_slots) and its draw counter k (TxChan::pad[1]) goes up by one; a channel that is not held keeps k.  It also
// writes on_air[c] = (lo, hi), the hull in columns of this pull of the tone samples the tile kernel rendered for the
// channel: read from the ring after the shift and before live_tx_commit retires anything, so it sees the starts the
// tile kernel rendered with.  The ring is in stream order, so lo comes from the first message whose tones meet the pull
// and hi from the last.
__global__ __launch_bounds__(256) void live_tx_commit_csma_kernel(TxChan* chan, TxDesc* desc, int32_t n, int32_t depth,
                                                                  int32_t T, const int32_t* lens, const int32_t* hold,
                                                                  int32_t holdoff, int32_t persist, int32_t slot,
                                                                  uint32_t seed, int32_t* pending, int64_t* deferred,
                                                                  int32_t* on_air) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    if (lens) {
        const int32_t l = lens[c];
        T = l < 0 ? 0 : (l < T ? l : T);
    }
    TxChan st = chan[c];
    const bool held = hold && hold[c] != 0;
    const int64_t earliest = tx_hold_earliest(st, T, held);
    TxDesc* ring = desc + (int64_t)c * depth;
    int64_t delta = 0;
    bool shifting = false;                                             // e is u or behind it
    int32_t lo = 0, hi = 0;
    for (int32_t i = 0, e = st.head; i < st.count; i++, e = (e + 1 == depth ? 0 : e + 1)) {
        TxDesc d = ring[e];
        if (!shifting && d.start >= st.pos) {                          // e is u
            shifting = true;
            delta = tx_hold_delta(earliest, d.start);
        }
        if (shifting && delta > 0) {
            d.start += delta;
            ring[e].start = d.start;
        }
        if (d.start >= st.pos + T) {
            if (delta == 0) break;                                     // nothing behind it moves or meets the pull
            continue;
        }
        const int64_t t1 = d.start + d.n_samples - AFSK_TAIL_SILENCE;  // the end of its tones
        if (t1 <= st.pos) continue;                                    // in its silent tail
        const int32_t a0 = (int32_t)(d.start > st.pos ? d.start - st.pos : 0);
        const int32_t a1 = (int32_t)(t1 < st.pos + T ? t1 - st.pos : T);
        if (hi == 0) lo = a0;                                          // (a1 > a0 >= 0: hi == 0 means none met yet)
        hi = a1;
    }
    st.end += delta;                                                   // (delta > 0: u is queued, so end >= u's end)
    const int32_t w = st.pad[0];
    if (held) {
        const uint32_t k = (uint32_t)st.pad[1];
        st.pad[0] = holdoff + slot * tx_csma_slots(seed, c, k, persist);   // < 2^31 by the entry's argument bounds
        st.pad[1] = (int32_t)(k + 1u);
    } else {
        st.pad[0] = w > T ? w - T : 0;
    }
    chan[c] = st;
    deferred[c] = delta;
    on_air[2 * c] = lo;
    on_air[2 * c + 1] = hi;
    live_tx_commit(chan, desc, c, depth, T, pending);
}

__global__ __launch_bounds__(256) void live_tx_reset_kernel(TxChan* chan, const uint8_t* mask, int32_t* pending,
                                                            int32_t n) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n && (!mask || mask[c])) {
        chan[c] = TxChan{};
        if (pending) pending[c] = 0;
    }
}

}  // namespace afsk

struct afsk_live_tx {
    afsk::DeviceState state;                    // the layout's L.bytes, live_tx_mixed_bytes(L), or R.bytes (rated)
    afsk::TxLayout L;
    int32_t bit_frames = 0, n_train_sym = 0;   // (a mixed transmitter: 0, see o_geom)
    int64_t o_geom = 0;                         // mixed: offset of TxGeom [n] in the state (0: uniform)
    int32_t n_rates = 0;                        // rated: entries of the table (0: not rated; then o_geom is 0 too)
    afsk::TxRatedLayout R;                      // rated: offsets of the table and of TxGeom [n, depth] in the state
};

namespace {

bool tx_bf_valid(int32_t bf) { return bf >= 4 && (bf & 3) == 0 && bf <= AFSK_SAMPLE_RATE; }
int tx_fail_bit_frames() {
    return afsk::fail(AFSK_E_INVALID_BAUD, "bit_frames must be a multiple of 4 in 4 ... 48000");
}
int64_t tx_train_sym(int32_t ts_cycles) { return 2 * (int64_t)(ts_cycles > 0 ? ts_cycles : 0); }   // ref:457
int tx_check_longest(int32_t bf, int64_t n_train_sym, int32_t max_payload_len) {
    const int64_t longest = (int64_t)bf * (n_train_sym + 4 + 14 * (int64_t)max_payload_len) + AFSK_TAIL_SILENCE;
    if (longest > AFSK_MAX_STREAM_LEN)
        return afsk::fail(AFSK_E_INVALID_ARG, "the longest message would exceed AFSK_MAX_STREAM_LEN samples");
    return AFSK_OK;
}

// afsk_live_tx_layout and afsk_live_tx_state_bytes_mixed: the state bytes of a uniform or a mixed transmitter
int tx_state_bytes(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len, bool mixed,
                   int64_t* out_state_bytes) {
    afsk::TxLayout L;
    if (int rc = afsk::live_tx_layout(n_channels, queue_depth, max_payload_len, L)) return rc;
    if (out_state_bytes) *out_state_bytes = mixed ? afsk::live_tx_mixed_bytes(L) : L.bytes;
    return AFSK_OK;
}

// Both create entries, after their own argument checks: bit_frames[c] / ts_cycles[c] per channel when `mixed`, else
// bit_frames[0] / ts_cycles[0] for every channel (the uniform transmitter).
int tx_create(int32_t n_channels, const int32_t* bit_frames, const int32_t* ts_cycles, bool mixed, int32_t queue_depth,
              int32_t max_payload_len, afsk_live_tx** out) {
    return afsk::no_throw([&] {
        std::unique_ptr<afsk_live_tx> tx(new afsk_live_tx());
        const afsk::TxLayout& L = tx->L;
        if (int rc = afsk::live_tx_layout(n_channels, queue_depth, max_payload_len, tx->L)) return rc;
        std::vector<afsk::TxGeom> geom(mixed ? (size_t)n_channels : 1);
        for (size_t c = 0; c < geom.size(); c++) {
            const int64_t nts = tx_train_sym(ts_cycles[c]);
            if (int rc = tx_check_longest(bit_frames[c], nts, max_payload_len)) return rc;
            geom[c] = afsk::TxGeom{bit_frames[c], (int32_t)nts};
        }
        tx->o_geom = mixed ? L.bytes : 0;
        if (!mixed) { tx->bit_frames = geom[0].bf; tx->n_train_sym = geom[0].n_train_sym; }
        // only the channel states (and the geometry) need a value: ring entries and payload slots are written before
        // they are read
        if (int rc = tx->state.create("afsk_live_tx_create", mixed ? afsk::live_tx_mixed_bytes(L) : L.bytes, L.o_desc,
                                      mixed ? geom.data() : nullptr, tx->o_geom, 8 * L.n))
            return rc;
        *out = tx.release();
        return AFSK_OK;
    });
}

int tx_check_n_rates(int32_t n_rates) {
    if (n_rates < 1 || n_rates > AFSK_DETECT_MAX_CANDIDATES)
        return afsk::fail(AFSK_E_INVALID_ARG, "n_rates must lie in 1 ... 36 (AFSK_DETECT_MAX_CANDIDATES)");
    return AFSK_OK;
}

// Both submit entries.  `rated_entry`: the call came through afsk_live_tx_submit_rated (a rated transmitter only); a
// rated transmitter's messages get rates[rate_index[i]], every one entry 0 with a null rate_index.
int tx_submit(afsk_live_tx* tx, bool rated_entry, int32_t n_msgs, const int32_t* channel, const int32_t* rate_index,
              const int64_t* payload_offset, const int32_t* payload_len, const uint8_t* payload,
              const int32_t* out_index, int32_t* out_status, int64_t* out_start, int32_t* out_n_samples,
              void* hip_stream) {
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, "null live transmitter");
    if (n_msgs < 0) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_msgs == 0) return AFSK_OK;
    if (!channel || !payload_offset || !payload_len || !payload || !out_status || !out_start || !out_n_samples)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (rated_entry && tx->n_rates == 0)
        return afsk::fail(AFSK_E_INVALID_ARG,
                          "afsk_live_tx_submit_rated needs a transmitter of afsk_live_tx_create_rated "
                          "(this one takes afsk_live_tx_submit)");
    if (int rc = tx->state.check_current()) return rc;
    const afsk::TxLayout& L = tx->L;
    uint8_t* d = tx->state.ptr();
    int32_t* first_bad = reinterpret_cast<int32_t*>(d + L.o_scratch);
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_tx_order_kernel, dim3(1), dim3(256), 0, st, channel, n_msgs, first_bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_tx_order_kernel");
    afsk::TxSubmitArgs a{};
    a.chan = reinterpret_cast<afsk::TxChan*>(d);
    a.desc = reinterpret_cast<afsk::TxDesc*>(d + L.o_desc);
    a.slots = d + L.o_slots;
    a.first_bad = first_bad;
    a.channel = channel;
    a.payload_offset = payload_offset;
    a.payload_len = payload_len;
    a.payload = payload;
    a.out_index = out_index;
    a.out_status = out_status;
    a.out_start = out_start;
    a.out_n_samples = out_n_samples;
    a.n_msgs = n_msgs;
    a.n = (int32_t)L.n;
    a.depth = (int32_t)L.depth;
    a.max_payload = (int32_t)L.max_payload;
    a.bf = tx->bit_frames;
    a.n_train_sym = tx->n_train_sym;
    a.geom = tx->o_geom ? reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom) : nullptr;
    const dim3 grid((uint32_t)((n_msgs + 255) / 256));
    if (tx->n_rates)
        hipLaunchKernelGGL(afsk::live_tx_submit_rated_kernel, grid, dim3(256), 0, st, a, rate_index,
                           reinterpret_cast<const afsk::TxGeom*>(d + tx->R.o_rates), tx->n_rates,
                           reinterpret_cast<afsk::TxGeom*>(d + tx->R.o_msg_geom));
    else
        hipLaunchKernelGGL(afsk::live_tx_submit_kernel, grid, dim3(256), 0, st, a);
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_tx_submit_kernel");
}

}  // namespace

extern "C" {

int afsk_live_tx_state_bytes_rated(int32_t n_channels, int32_t n_rates, int32_t queue_depth, int32_t max_payload_len,
                                   int64_t* out_state_bytes) {
    afsk::TxLayout L;
    if (int rc = afsk::live_tx_layout(n_channels, queue_depth, max_payload_len, L)) return rc;
    if (int rc = tx_check_n_rates(n_rates)) return rc;
    if (out_state_bytes) *out_state_bytes = afsk::live_tx_rated_layout(L, n_rates).bytes;
    return AFSK_OK;
}

int afsk_live_tx_create_rated(int32_t n_channels, int32_t n_rates, const int32_t* bit_frames_host,
                              const int32_t* ts_cycles_host, int32_t queue_depth, int32_t max_payload_len,
                              afsk_live_tx** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (int rc = tx_check_n_rates(n_rates)) return rc;
    if (!bit_frames_host || !ts_cycles_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t r = 0; r < n_rates; r++)
        if (!tx_bf_valid(bit_frames_host[r])) return tx_fail_bit_frames();
    return afsk::no_throw([&] {
        std::unique_ptr<afsk_live_tx> tx(new afsk_live_tx());
        const afsk::TxLayout& L = tx->L;
        if (int rc = afsk::live_tx_layout(n_channels, queue_depth, max_payload_len, tx->L)) return rc;
        std::vector<afsk::TxGeom> table((size_t)n_rates);
        for (int32_t r = 0; r < n_rates; r++) {
            const int64_t nts = tx_train_sym(ts_cycles_host[r]);
            if (int rc = tx_check_longest(bit_frames_host[r], nts, max_payload_len)) return rc;
            table[r] = afsk::TxGeom{bit_frames_host[r], (int32_t)nts};
        }
        tx->n_rates = n_rates;
        tx->R = afsk::live_tx_rated_layout(L, n_rates);
        // the channel states and the table need a value: a ring entry and its geometry are written by the submit that
        // queues the message, and a pull reads only entries in [head, head + count)
        if (int rc = tx->state.create("afsk_live_tx_create_rated", tx->R.bytes, L.o_desc, table.data(), tx->R.o_rates,
                                      8 * (int64_t)n_rates))
            return rc;
        *out = tx.release();
        return AFSK_OK;
    });
}

int afsk_live_tx_layout(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len, int64_t* out_state_bytes) {
    return tx_state_bytes(n_channels, queue_depth, max_payload_len, false, out_state_bytes);
}

int afsk_live_tx_state_bytes_mixed(int32_t n_channels, int32_t queue_depth, int32_t max_payload_len,
                                   int64_t* out_state_bytes) {
    return tx_state_bytes(n_channels, queue_depth, max_payload_len, true, out_state_bytes);
}

int afsk_live_tx_create(int32_t n_channels, int32_t bit_frames, int32_t ts_cycles, int32_t queue_depth,
                        int32_t max_payload_len, afsk_live_tx** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (!tx_bf_valid(bit_frames)) return tx_fail_bit_frames();
    return tx_create(n_channels, &bit_frames, &ts_cycles, false, queue_depth, max_payload_len, out);
}

int afsk_live_tx_create_mixed(int32_t n_channels, const int32_t* bit_frames_host, const int32_t* ts_cycles_host,
                              int32_t queue_depth, int32_t max_payload_len, afsk_live_tx** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out = nullptr;
    if (n_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, "n_channels must be at least 1");
    if (!bit_frames_host || !ts_cycles_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t c = 0; c < n_channels; c++)
        if (!tx_bf_valid(bit_frames_host[c])) return tx_fail_bit_frames();
    bool same = true;
    for (int32_t c = 1; c < n_channels && same; c++)
        same = bit_frames_host[c] == bit_frames_host[0] && tx_train_sym(ts_cycles_host[c]) == tx_train_sym(ts_cycles_host[0]);
    // one geometry for every channel: the uniform transmitter (its launches, its state bytes)
    return tx_create(n_channels, bit_frames_host, ts_cycles_host, !same, queue_depth, max_payload_len, out);
}

int afsk_live_tx_info(const afsk_live_tx* tx, int32_t* out_n_channels, int32_t* out_queue_depth,
                      int32_t* out_max_payload_len, int64_t* out_state_bytes) {
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, "null live transmitter");
    if (out_n_channels) *out_n_channels = (int32_t)tx->L.n;
    if (out_queue_depth) *out_queue_depth = (int32_t)tx->L.depth;
    if (out_max_payload_len) *out_max_payload_len = (int32_t)tx->L.max_payload;
    if (out_state_bytes) *out_state_bytes = tx->state.bytes;
    return AFSK_OK;
}

int afsk_live_tx_submit(afsk_live_tx* tx, int32_t n_msgs, const int32_t* channel, const int64_t* payload_offset,
                        const int32_t* payload_len, const uint8_t* payload, const int32_t* out_index,
                        int32_t* out_status, int64_t* out_start, int32_t* out_n_samples, void* hip_stream) {
    return tx_submit(tx, false, n_msgs, channel, nullptr, payload_offset, payload_len, payload, out_index, out_status,
                     out_start, out_n_samples, hip_stream);
}

int afsk_live_tx_submit_rated(afsk_live_tx* tx, int32_t n_msgs, const int32_t* channel, const int32_t* rate_index,
                              const int64_t* payload_offset, const int32_t* payload_len, const uint8_t* payload,
                              const int32_t* out_index, int32_t* out_status, int64_t* out_start,
                              int32_t* out_n_samples, void* hip_stream) {
    return tx_submit(tx, true, n_msgs, channel, rate_index, payload_offset, payload_len, payload, out_index, out_status,
                     out_start, out_n_samples, hip_stream);
}

namespace {

// What afsk_live_tx_pull_hold adds to a pull's arguments (a null TxHold: the plain or ragged pull).
struct TxHold {
    const int32_t* hold;        // DEVICE int32 [n] or NULL (nobody held)
    int32_t holdoff;
    int64_t* deferred;
    bool csma = false;          // afsk_live_tx_pull_csma: the four below, and the csma commit
    int32_t persist = 255, slot = 0;
    uint32_t seed = 0;
    int32_t* on_air = nullptr;
};

// afsk_live_tx_pull, afsk_live_tx_pull_ragged (`ragged`: the ragged kernels, lens a DEVICE array or NULL) and
// afsk_live_tx_pull_hold (`hd`: the hold kernels, which are ragged ones) and afsk_live_tx_pull_csma (`hd->csma`: the hold
// tile kernels and the csma commit)
int tx_pull(afsk_live_tx* tx, int16_t* out, int64_t out_row_stride, int32_t n_samples, bool ragged, const int32_t* lens,
            int32_t* out_pending, void* hip_stream, const TxHold* hd = nullptr) {
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, "null live transmitter");
    if (hd && (hd->holdoff < 0 || hd->holdoff > AFSK_MAX_STREAM_LEN))
        return afsk::fail(AFSK_E_INVALID_ARG, "holdoff must lie in 0 ... AFSK_MAX_STREAM_LEN");
    if (hd && !hd->deferred) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument (out_deferred)");
    if (hd && hd->csma) {
        if (hd->persist < 0 || hd->persist > 255)
            return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_tx_pull_csma: persist must lie in 0 ... 255");
        if (hd->slot < 0 || hd->slot > (1 << 20))
            return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_tx_pull_csma: slot must lie in 0 ... 2^20");
        if (!hd->on_air) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_tx_pull_csma: null pointer argument (out_on_air)");
    }
    if (n_samples < 0 || out_row_stride < 0) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_samples > AFSK_MAX_STREAM_LEN) return afsk::fail(AFSK_E_INVALID_ARG, "n_samples exceeds AFSK_MAX_STREAM_LEN");
    const afsk::TxLayout& L = tx->L;
    if (L.n > 1 && n_samples > 0 && out_row_stride < n_samples)
        return afsk::fail(AFSK_E_INVALID_ARG, "out_row_stride below n_samples: the rows would overlap");
    if ((n_samples > 0 && !out) || !out_pending) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const int32_t tiles = (int32_t)((n_samples + afsk::kTxTile - 1) / afsk::kTxTile);
    if ((int64_t)tiles * L.n > 0x7fffffffll) return afsk::fail(AFSK_E_INVALID_ARG, "n_channels * tiles exceeds 2^31 - 1");
    if (int rc = tx->state.check_current()) return rc;
    uint8_t* d = tx->state.ptr();
    afsk::TxChan* chan = reinterpret_cast<afsk::TxChan*>(d);
    const afsk::TxDesc* desc = reinterpret_cast<const afsk::TxDesc*>(d + L.o_desc);
    const hipStream_t st = (hipStream_t)hip_stream;
    hipError_t e;
    if (n_samples > 0) {
        afsk::TxPullArgs a{};
        a.chan = chan;
        a.desc = desc;
        a.slots = d + L.o_slots;
        a.out = out;
        a.out_stride = out_row_stride;
        a.T = n_samples;
        a.tiles = tiles;
        // several consecutive tiles per block share the loads of the channel state and ring, as long as the grid keeps
        // at least 32 waves per CU
        const int64_t all = (int64_t)tiles * L.n;
        a.tiles_per_block = all >= 4 * afsk::kTxMinBlocks ? 4 : (all >= 2 * afsk::kTxMinBlocks ? 2 : 1);
        a.blocks_per_row = (tiles + a.tiles_per_block - 1) / a.tiles_per_block;
        a.depth = (int32_t)L.depth;
        a.max_payload = (int32_t)L.max_payload;
        a.bf = (uint32_t)tx->bit_frames;
        a.n_train_sym = (uint32_t)tx->n_train_sym;
        const dim3 grid((uint32_t)(a.blocks_per_row * L.n));
        const afsk::TxGeom* msg_geom = reinterpret_cast<const afsk::TxGeom*>(d + tx->R.o_msg_geom);   // (rated)
        if (hd && tx->n_rates)
            hipLaunchKernelGGL(afsk::live_tx_tile_hold_kernel_rated, grid, dim3(afsk::kTxThreads), 0, st, a, msg_geom,
                               lens, hd->hold);
        else if (hd && tx->o_geom)
            hipLaunchKernelGGL(afsk::live_tx_tile_hold_kernel_mixed, grid, dim3(afsk::kTxThreads), 0, st, a,
                               reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom), lens, hd->hold);
        else if (hd && tx->bit_frames / 4 >= 8)
            hipLaunchKernelGGL(afsk::live_tx_tile_hold_kernel<false>, grid, dim3(afsk::kTxThreads), 0, st, a, lens,
                               hd->hold);
        else if (hd)
            hipLaunchKernelGGL(afsk::live_tx_tile_hold_kernel<true>, grid, dim3(afsk::kTxThreads), 0, st, a, lens,
                               hd->hold);
        else if (ragged && tx->n_rates)
            hipLaunchKernelGGL(afsk::live_tx_tile_ragged_kernel_rated, grid, dim3(afsk::kTxThreads), 0, st, a, msg_geom,
                               lens);
        else if (tx->n_rates)
            hipLaunchKernelGGL(afsk::live_tx_tile_kernel_rated, grid, dim3(afsk::kTxThreads), 0, st, a, msg_geom);
        else if (ragged && tx->o_geom)
            hipLaunchKernelGGL(afsk::live_tx_tile_ragged_kernel_mixed, grid, dim3(afsk::kTxThreads), 0, st, a,
                               reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom), lens);
        else if (ragged && tx->bit_frames / 4 >= 8)
            hipLaunchKernelGGL(afsk::live_tx_tile_ragged_kernel<false>, grid, dim3(afsk::kTxThreads), 0, st, a, lens);
        else if (ragged)
            hipLaunchKernelGGL(afsk::live_tx_tile_ragged_kernel<true>, grid, dim3(afsk::kTxThreads), 0, st, a, lens);
        else if (tx->o_geom)
            hipLaunchKernelGGL(afsk::live_tx_tile_kernel_mixed, grid, dim3(afsk::kTxThreads), 0, st, a,
                               reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom));
        else if (tx->bit_frames / 4 >= 8) hipLaunchKernelGGL(afsk::live_tx_tile_kernel<false>, grid, dim3(afsk::kTxThreads), 0, st, a);
        else hipLaunchKernelGGL(afsk::live_tx_tile_kernel<true>, grid, dim3(afsk::kTxThreads), 0, st, a);
        e = hipGetLastError();
        if (e != hipSuccess) return afsk::hip_fail(e, "launch live_tx_tile_kernel");
    }
    if (hd && hd->csma)
        hipLaunchKernelGGL(afsk::live_tx_commit_csma_kernel, dim3((uint32_t)((L.n + 255) / 256)), dim3(256), 0, st,
                           chan, reinterpret_cast<afsk::TxDesc*>(d + L.o_desc), (int32_t)L.n, (int32_t)L.depth,
                           n_samples, lens, hd->hold, hd->holdoff, hd->persist, hd->slot, hd->seed, out_pending,
                           hd->deferred, hd->on_air);
    else if (hd)
        hipLaunchKernelGGL(afsk::live_tx_commit_hold_kernel, dim3((uint32_t)((L.n + 255) / 256)), dim3(256), 0, st,
                           chan, reinterpret_cast<afsk::TxDesc*>(d + L.o_desc), (int32_t)L.n, (int32_t)L.depth,
                           n_samples, lens, hd->hold, hd->holdoff, out_pending, hd->deferred);
    else if (ragged)
        hipLaunchKernelGGL(afsk::live_tx_commit_ragged_kernel, dim3((uint32_t)((L.n + 255) / 256)), dim3(256), 0, st,
                           chan, desc, (int32_t)L.n, (int32_t)L.depth, n_samples, lens, out_pending);
    else
        hipLaunchKernelGGL(afsk::live_tx_commit_kernel, dim3((uint32_t)((L.n + 255) / 256)), dim3(256), 0, st, chan, desc,
                           (int32_t)L.n, (int32_t)L.depth, n_samples, out_pending);
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_tx_commit_kernel");
}

}  // namespace

int afsk_live_tx_pull(afsk_live_tx* tx, int16_t* out, int64_t out_row_stride, int32_t n_samples, int32_t* out_pending,
                      void* hip_stream) {
    return tx_pull(tx, out, out_row_stride, n_samples, false, nullptr, out_pending, hip_stream);
}

int afsk_live_tx_pull_ragged(afsk_live_tx* tx, int16_t* out, int64_t out_row_stride, int32_t n_samples,
                             const int32_t* d_lens_or_null, int32_t* out_pending, void* hip_stream) {
    return tx_pull(tx, out, out_row_stride, n_samples, true, d_lens_or_null, out_pending, hip_stream);
}

int afsk_live_tx_pull_hold(afsk_live_tx* tx, int16_t* out, int64_t out_row_stride, int32_t n_samples,
                           const int32_t* d_lens_or_null, const int32_t* d_hold_or_null, int32_t holdoff,
                           int32_t* out_pending, int64_t* out_deferred, void* hip_stream) {
    const TxHold hd{d_hold_or_null, holdoff, out_deferred};
    return tx_pull(tx, out, out_row_stride, n_samples, true, d_lens_or_null, out_pending, hip_stream, &hd);
}

int afsk_live_tx_pull_csma(afsk_live_tx* tx, int16_t* out, int64_t out_row_stride, int32_t n_samples,
                           const int32_t* d_lens_or_null, const int32_t* d_hold_or_null, int32_t holdoff,
                           int32_t persist, int32_t slot, uint32_t seed, int32_t* out_pending, int64_t* out_deferred,
                           int32_t* out_on_air, void* hip_stream) {
    const TxHold hd{d_hold_or_null, holdoff, out_deferred, true, persist, slot, seed, out_on_air};
    return tx_pull(tx, out, out_row_stride, n_samples, true, d_lens_or_null, out_pending, hip_stream, &hd);
}

int afsk_live_tx_reset(afsk_live_tx* tx, const uint8_t* d_mask_or_null, int32_t* out_pending_or_null,
                       void* hip_stream) {
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, "null live transmitter");
    if (int rc = tx->state.check_current()) return rc;
    hipLaunchKernelGGL(afsk::live_tx_reset_kernel, dim3((uint32_t)((tx->L.n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)hip_stream, static_cast<afsk::TxChan*>(tx->state.d), d_mask_or_null, out_pending_or_null,
                       (int32_t)tx->L.n);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_tx_reset_kernel");
}

int afsk_live_tx_destroy(afsk_live_tx* tx) {
    delete tx;        // the caller has synchronised the launches that use it
    return AFSK_OK;
}

}  // extern "C"
