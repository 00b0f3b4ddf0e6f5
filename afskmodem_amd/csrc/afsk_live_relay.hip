// afsk_live_relay.hip -- the relay submit of the live transmitter (afsk_live_relay_check_map,
// afsk_live_tx_submit_events, include/afsk_amd.h): the bursts a push closed, as afsk_live_pack left them in its events
// buffer on the device, queued on a live transmitter where they lie -- no copy to the host, no host read of a count.
//
// A call is two launches in order on the caller's stream:
//   live_relay_order_kernel  ONE block of kOrderThreads: reads `stored` from the header, clamps it to 0 ... max_events
//                            and finds the first stored record whose channel is below its predecessor's (the guard of
//                            afsk_live_tx_submit; a real pack never trips it).  Both values go to the transmitter's
//                            submit scratch.
//   live_relay_kernel        one wave per kRelayPerWave consecutive record indices.  An index at or past `stored`
//                            gets AFSK_LIVE_TX_NONE, one at or past the first unsorted record AFSK_LIVE_TX_UNSORTED.  A
//                            record that is not the first of its run of equal channels is left to the wave that holds
//                            the first one.  That wave walks the run: every value it decides on is the same in all 64
//                            lanes (the record, the map entry, the channel state), lane 0 writes the outputs, the ring
//                            entry and the channel state, and all 64 lanes copy a queued payload.  Every store is a
//                            plain vector store; there is no atomic and no LDS.
// Records of one channel form one run in front of the first unsorted record, so one wave alone reads and writes the
// state of a destination channel as long as no two receiver channels name it (afsk_live_relay_check_map).
//
// The payload copy (relay_copy) is the packer's: single bytes up to the destination's next 16-byte boundary, 16-byte
// stores fed by 16-byte loads of any alignment, single bytes for the rest.  Every load lies inside the payload's own
// bytes, every store inside the message's slot.
//
// What the kernels read of the events buffer: the header's `stored`, the first `stored` records (of a record at or
// past the first unsorted one its channel alone), the payload bytes of queued records.  A payload range is checked
// against [0, max_bytes) before a byte of it is read.  Nothing of the events buffer is written.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end), behind
// afsk_live_tx.hip, whose TxChan / TxDesc / TxGeom / TxLayout and afsk_live_tx it uses.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace afsk {

constexpr int kRelayThreads = 256;                              // 4 waves per block
constexpr int kRelayPerWave = 4;                                // record indices per wave
constexpr int kRelayPerBlock = kRelayThreads / 64 * kRelayPerWave;
constexpr int kOrderThreads = 1024;                             // live_relay_order_kernel: one block of 16 waves
constexpr int kOrderUnroll = 8;                                 // pairs a thread loads per step
constexpr int64_t kRelayHeaderBytes = 32;                       // the header of a packed list (afsk_live_pack.hip)
static_assert(sizeof(afsk_live_event) == 48, "afsk_live_event is 48 bytes without padding");

typedef uint32_t relay_vec16 __attribute__((ext_vector_type(4)));
typedef uint32_t relay_vec16_u __attribute__((ext_vector_type(4), aligned(1)));   // a payload starts at any byte

// What live_relay_kernel only reads -- no store of the kernel writes it, so it comes as __restrict__ parameters: the
// loads may be scalar and may move ahead of the stores.
struct RelayInputs {
    const int32_t* scratch;         // [0] the first unsorted record (`stored`: none), [1] `stored`, clamped
    const afsk_live_event* records;
    const uint8_t* payload;
    const int32_t* map;             // NULL: the identity
    const TxGeom* geom;             // mixed: per-channel bf / n_train_sym (NULL: RelayArgs' two)
};

struct RelayArgs {
    TxChan* chan;
    TxDesc* desc;
    uint8_t* slots;
    int32_t* out_status;
    int64_t* out_start;
    int32_t* out_n_samples;
    int32_t max_events;
    int32_t max_bytes;
    int32_t out_stride;
    int32_t n_rx;
    int32_t skip_flags;             // AFSK_LIVE_OVERFLOW included
    int32_t n;
    int32_t depth;
    int32_t max_payload;
    int32_t bf;
    int32_t n_train_sym;
};

// One block.  A thread looks at the pairs (i - 1, i) for i = tid + 1, tid + 1 + kOrderThreads, ...: kOrderUnroll of
// them per step, their 2 * kOrderUnroll loads issued together, and stops at the first step that holds a descending
// pair (a thread's indices rise, so its first find is its least).
__global__ __launch_bounds__(kOrderThreads) void live_relay_order_kernel(const int32_t* __restrict__ header,
                                                                         const afsk_live_event* __restrict__ records,
                                                                         int32_t max_events, int32_t* scratch) {
    __shared__ int32_t red[kOrderThreads];
    const int32_t stored = min(max(header[1], 0), max_events);
    int32_t m = stored;
    for (int64_t i0 = (int64_t)threadIdx.x + 1; i0 < stored; i0 += (int64_t)kOrderThreads * kOrderUnroll) {
        // (a pair past the list is read at the list's last pair instead, so that no load waits for a bounds branch)
        int32_t cur[kOrderUnroll], prev[kOrderUnroll];
#pragma unroll
        for (int u = 0; u < kOrderUnroll; u++) {
            const int64_t i = min(i0 + (int64_t)u * kOrderThreads, (int64_t)stored - 1);
            cur[u] = records[i].channel;
            prev[u] = records[i - 1].channel;
        }
        int32_t found = stored;
#pragma unroll
        for (int u = kOrderUnroll - 1; u >= 0; u--) {           // downwards: the least index is written last
            const int64_t i = i0 + (int64_t)u * kOrderThreads;
            if (i < stored && cur[u] < prev[u]) found = (int32_t)i;
        }
        if (found < stored) { m = found; break; }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = kOrderThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scratch[0] = red[0];
        scratch[1] = stored;
    }
}

// len bytes from src to dst by the whole wave; the ranges do not overlap
__device__ __forceinline__ void relay_copy(uint8_t* dst, const uint8_t* src, int32_t len, int lane) {
    const int32_t head = min((int32_t)((16 - ((uintptr_t)dst & 15)) & 15), len);
    if (lane < head) dst[lane] = src[lane];
    const int32_t body = (len - head) >> 4;
    for (int32_t i = lane; i < body; i += 64)
        *reinterpret_cast<relay_vec16*>(dst + head + 16 * (int64_t)i) =
            *reinterpret_cast<const relay_vec16_u*>(src + head + 16 * (int64_t)i);
    const int32_t done = head + 16 * body;
    if (lane < len - done) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(kRelayThreads) void live_relay_kernel(RelayArgs a, const int32_t* __restrict__ scratch,
                                                                   const afsk_live_event* __restrict__ records,
                                                                   const uint8_t* __restrict__ payload,
                                                                   const int32_t* __restrict__ map,
                                                                   const TxGeom* __restrict__ geom) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = ((int64_t)blockIdx.x * (kRelayThreads / 64) + wave) * kRelayPerWave;
    if (base >= a.max_events) return;
    const int32_t first_bad = scratch[0];
    const int32_t stored = scratch[1];
    auto put = [&](int32_t j, int32_t status, int64_t start, int32_t ns) {
        if (lane == 0) {
            a.out_status[j] = status;
            a.out_start[j] = start;
            a.out_n_samples[j] = ns;
        }
    };
    for (int k = 0; k < kRelayPerWave; k++) {
        const int32_t i = (int32_t)base + k;
        if (i >= a.max_events) break;
        if (i >= stored) { put(i, AFSK_LIVE_TX_NONE, -1, 0); continue; }
        if (i >= first_bad) { put(i, AFSK_LIVE_TX_UNSORTED, -1, 0); continue; }
        const int32_t ch = records[i].channel;
        if (i > 0 && records[i - 1].channel == ch) continue;      // not the first of its run
        // the run's destination channel; the map is read for a channel of the receiver alone
        int32_t dst = ch;
        bool dropped = false;
        if (map) {
            const bool in_rx = ch >= 0 && ch < a.n_rx;
            dst = in_rx ? map[ch] : -1;
            dropped = in_rx && dst < 0;
        }
        const bool ok = dst >= 0 && dst < a.n;
        TxChan st = ok ? a.chan[dst] : TxChan{};
        const TxGeom g = ok && geom ? geom[dst] : TxGeom{a.bf, a.n_train_sym};
        for (int32_t j = i; j < first_bad && records[j].channel == ch; j++) {
            const afsk_live_event r = records[j];
            const int64_t off = r.payload_offset;
            if ((r.flags & a.skip_flags) != 0 || r.status != AFSK_ST_OK || r.nbytes < 1 || r.nbytes > a.out_stride ||
                off < 0 || off + r.nbytes > a.max_bytes || dropped) {
                put(j, AFSK_LIVE_TX_SKIPPED, -1, 0);
                continue;
            }
            const int32_t plen = r.nbytes;
            if (!ok) { put(j, AFSK_LIVE_TX_BAD_CHANNEL, -1, 0); continue; }
            if (plen > a.max_payload) { put(j, AFSK_LIVE_TX_TOO_LONG, -1, 0); continue; }
            if (st.count >= a.depth) { put(j, AFSK_LIVE_TX_QUEUE_FULL, -1, 0); continue; }
            const int64_t start = st.pos > st.end ? st.pos : st.end;
            const int32_t ns = g.bf * (g.n_train_sym + 4 + 14 * plen) + AFSK_TAIL_SILENCE;   // <= AFSK_MAX_STREAM_LEN
            int32_t slot = st.head + st.count;
            if (slot >= a.depth) slot -= a.depth;
            const int64_t e = (int64_t)dst * a.depth + slot;
            if (lane == 0) a.desc[e] = TxDesc{start, ns, plen};
            relay_copy(a.slots + e * a.max_payload, payload + off, plen, lane);
            st.end = start + ns;
            st.count++;
            put(j, AFSK_LIVE_TX_QUEUED, start, ns);
        }
        if (ok && lane == 0) a.chan[dst] = st;
    }
}

// What the rated relay adds (a rated transmitter, afsk_live_tx_submit_events_rated): the table, the geometry ring it
// writes next to the descriptors, and the rates the auto receiver's push left -- int32 [n_rx, rx_slots], entry
// (channel, slot) of a record its burst's bit_frames.  A null rx_bf: every record plays at table entry 0.
struct RelayRated {
    const TxGeom* rates;
    TxGeom* msg_geom;
    const int32_t* rx_bf;
    int32_t n_rates;
    int32_t rx_slots;
};

// live_relay_kernel for a rated transmitter (kept a kernel of its own: the one above is the code it was): the record's
// rate is looked up in the table (the first entry with its bit_frames; none: AFSK_LIVE_TX_BAD_RATE, behind _TOO_LONG
// and in front of _QUEUE_FULL), a record whose (channel, slot) lies outside the rate array is AFSK_LIVE_TX_SKIPPED
// before the array is read, and a queued message's geometry goes to msg_geom next to its descriptor.
__global__ __launch_bounds__(kRelayThreads) void live_relay_rated_kernel(RelayArgs a, RelayRated rated,
                                                                         const int32_t* __restrict__ scratch,
                                                                         const afsk_live_event* __restrict__ records,
                                                                         const uint8_t* __restrict__ payload,
                                                                         const int32_t* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = ((int64_t)blockIdx.x * (kRelayThreads / 64) + wave) * kRelayPerWave;
    if (base >= a.max_events) return;
    const int32_t first_bad = scratch[0];
    const int32_t stored = scratch[1];
    auto put = [&](int32_t j, int32_t status, int64_t start, int32_t ns) {
        if (lane == 0) {
            a.out_status[j] = status;
            a.out_start[j] = start;
            a.out_n_samples[j] = ns;
        }
    };
    for (int k = 0; k < kRelayPerWave; k++) {
        const int32_t i = (int32_t)base + k;
        if (i >= a.max_events) break;
        if (i >= stored) { put(i, AFSK_LIVE_TX_NONE, -1, 0); continue; }
        if (i >= first_bad) { put(i, AFSK_LIVE_TX_UNSORTED, -1, 0); continue; }
        const int32_t ch = records[i].channel;
        if (i > 0 && records[i - 1].channel == ch) continue;      // not the first of its run
        // the run's destination channel; the map is read for a channel of the receiver alone
        int32_t dst = ch;
        bool dropped = false;
        if (map) {
            const bool in_rx = ch >= 0 && ch < a.n_rx;
            dst = in_rx ? map[ch] : -1;
            dropped = in_rx && dst < 0;
        }
        const bool ok = dst >= 0 && dst < a.n;
        TxChan st = ok ? a.chan[dst] : TxChan{};
        for (int32_t j = i; j < first_bad && records[j].channel == ch; j++) {
            const afsk_live_event r = records[j];
            const int64_t off = r.payload_offset;
            // (the last line: no place in the rate array -- decided before the array is read)
            if ((r.flags & a.skip_flags) != 0 || r.status != AFSK_ST_OK || r.nbytes < 1 || r.nbytes > a.out_stride ||
                off < 0 || off + r.nbytes > a.max_bytes || dropped ||
                (rated.rx_bf && (ch < 0 || ch >= a.n_rx || r.slot < 0 || r.slot >= rated.rx_slots))) {
                put(j, AFSK_LIVE_TX_SKIPPED, -1, 0);
                continue;
            }
            const int32_t plen = r.nbytes;
            if (!ok) { put(j, AFSK_LIVE_TX_BAD_CHANNEL, -1, 0); continue; }
            if (plen > a.max_payload) { put(j, AFSK_LIVE_TX_TOO_LONG, -1, 0); continue; }
            int32_t idx = 0;                                      // the first table entry at the rate heard
            if (rated.rx_bf) {
                const int32_t heard = rated.rx_bf[(int64_t)ch * rated.rx_slots + r.slot];
                while (idx < rated.n_rates && rated.rates[idx].bf != heard) idx++;
            }
            if (idx >= rated.n_rates) { put(j, AFSK_LIVE_TX_BAD_RATE, -1, 0); continue; }
            const TxGeom g = rated.rates[idx];
            if (st.count >= a.depth) { put(j, AFSK_LIVE_TX_QUEUE_FULL, -1, 0); continue; }
            const int64_t start = st.pos > st.end ? st.pos : st.end;
            const int32_t ns = g.bf * (g.n_train_sym + 4 + 14 * plen) + AFSK_TAIL_SILENCE;   // <= AFSK_MAX_STREAM_LEN
            int32_t slot = st.head + st.count;
            if (slot >= a.depth) slot -= a.depth;
            const int64_t e = (int64_t)dst * a.depth + slot;
            if (lane == 0) {
                a.desc[e] = TxDesc{start, ns, plen};
                rated.msg_geom[e] = g;
            }
            relay_copy(a.slots + e * a.max_payload, payload + off, plen, lane);
            st.end = start + ns;
            st.count++;
            put(j, AFSK_LIVE_TX_QUEUED, start, ns);
        }
        if (ok && lane == 0) a.chan[dst] = st;
    }
}

}  // namespace afsk

extern "C" {

int afsk_live_relay_check_map(const int32_t* map_host, int32_t n_rx_channels, int32_t n_tx_channels) {
    if (n_rx_channels < 1 || n_tx_channels < 1)
        return afsk::fail(AFSK_E_INVALID_ARG, "n_rx_channels and n_tx_channels must be at least 1");
    if (!map_host) return AFSK_OK;                               // the identity
    return afsk::no_throw([&] {
        // (destination, receiver channel) of every entry that names a transmitter channel, sorted: equal destinations
        // become neighbours, the lower receiver channel first
        std::vector<std::pair<int32_t, int32_t>> named;
        for (int32_t c = 0; c < n_rx_channels; c++)
            if (map_host[c] >= 0 && map_host[c] < n_tx_channels) named.emplace_back(map_host[c], c);
        std::sort(named.begin(), named.end());
        for (size_t i = 1; i < named.size(); i++)
            if (named[i].first == named[i - 1].first)
                return afsk::fail(AFSK_E_INVALID_ARG,
                                  "receiver channels " + std::to_string(named[i - 1].second) + " and " +
                                      std::to_string(named[i].second) + " both map to transmitter channel " +
                                      std::to_string(named[i].first) +
                                      ": a transmitter channel takes the bursts of one receiver channel");
        return (int)AFSK_OK;
    });
}

namespace {

// Both relay entries.  `rated_entry`: the call came through afsk_live_tx_submit_events_rated (a rated transmitter
// only), rx_bf / rx_slots its rate array; a rated transmitter served through afsk_live_tx_submit_events plays every
// record at table entry 0 (rx_bf null).
int relay_submit(afsk_live_tx* tx, bool rated_entry, const void* events, int32_t max_events, int32_t max_bytes,
                 int32_t out_stride, int32_t n_rx_channels, const int32_t* d_channel_map_or_null, int32_t skip_flags,
                 const int32_t* rx_bf, int32_t rx_slots, int32_t* out_status, int64_t* out_start,
                 int32_t* out_n_samples, void* hip_stream) {
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, "null live transmitter");
    if (max_events < 0 || max_bytes < 0 || out_stride < 0) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_rx_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, "n_rx_channels must be at least 1");
    // (afsk_live_events_layout's bound n_channels * slots < 2^31 holds for every int32 n_rx_channels at slots >= 1)
    if (skip_flags & ~(AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW))
        return afsk::fail(AFSK_E_INVALID_ARG, "skip_flags may hold AFSK_LIVE_OPEN_END and AFSK_LIVE_OVERFLOW alone");
    if (!events || !out_status || !out_start || !out_n_samples)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (rated_entry && (!rx_bf || rx_slots < 1))
        return afsk::fail(AFSK_E_INVALID_ARG, "d_rx_bit_frames must not be NULL and rx_slots must be at least 1");
    if (rated_entry && tx->n_rates == 0)
        return afsk::fail(AFSK_E_INVALID_ARG,
                          "afsk_live_tx_submit_events_rated needs a transmitter of afsk_live_tx_create_rated "
                          "(this one takes afsk_live_tx_submit_events)");
    if ((uintptr_t)events & 15) return afsk::fail(AFSK_E_INVALID_ARG, "the events buffer must be 16-byte aligned");
    if (max_events == 0) return AFSK_OK;
    if (int rc = tx->state.check_current()) return rc;
    const afsk::TxLayout& L = tx->L;
    uint8_t* d = tx->state.ptr();
    const uint8_t* ev = static_cast<const uint8_t*>(events);
    afsk::RelayArgs a{};
    a.chan = reinterpret_cast<afsk::TxChan*>(d);
    a.desc = reinterpret_cast<afsk::TxDesc*>(d + L.o_desc);
    a.slots = d + L.o_slots;
    int32_t* scratch = reinterpret_cast<int32_t*>(d + L.o_scratch);
    afsk::RelayInputs in{};
    in.scratch = scratch;
    in.records = reinterpret_cast<const afsk_live_event*>(ev + afsk::kRelayHeaderBytes);
    in.payload = ev + afsk::kRelayHeaderBytes + (int64_t)sizeof(afsk_live_event) * max_events;
    in.map = d_channel_map_or_null;
    in.geom = tx->o_geom ? reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom) : nullptr;
    a.out_status = out_status;
    a.out_start = out_start;
    a.out_n_samples = out_n_samples;
    a.max_events = max_events;
    a.max_bytes = max_bytes;
    a.out_stride = out_stride;
    a.n_rx = n_rx_channels;
    a.skip_flags = skip_flags | AFSK_LIVE_OVERFLOW;
    a.n = (int32_t)L.n;
    a.depth = (int32_t)L.depth;
    a.max_payload = (int32_t)L.max_payload;
    a.bf = tx->bit_frames;
    a.n_train_sym = tx->n_train_sym;
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_relay_order_kernel, dim3(1), dim3(afsk::kOrderThreads), 0, st,
                       reinterpret_cast<const int32_t*>(ev) /* the header: [1] is `stored` */, in.records, max_events,
                       scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_relay_order_kernel");
    const uint32_t blocks = (uint32_t)(((int64_t)max_events + afsk::kRelayPerBlock - 1) / afsk::kRelayPerBlock);
    if (tx->n_rates) {
        afsk::RelayRated rated{};
        rated.rates = reinterpret_cast<const afsk::TxGeom*>(d + tx->R.o_rates);
        rated.msg_geom = reinterpret_cast<afsk::TxGeom*>(d + tx->R.o_msg_geom);
        rated.rx_bf = rx_bf;
        rated.n_rates = tx->n_rates;
        rated.rx_slots = rx_slots;
        hipLaunchKernelGGL(afsk::live_relay_rated_kernel, dim3(blocks), dim3(afsk::kRelayThreads), 0, st, a, rated,
                           in.scratch, in.records, in.payload, in.map);
    } else {
        hipLaunchKernelGGL(afsk::live_relay_kernel, dim3(blocks), dim3(afsk::kRelayThreads), 0, st, a, in.scratch,
                           in.records, in.payload, in.map, in.geom);
    }
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_relay_kernel");
}

}  // namespace

int afsk_live_tx_submit_events(afsk_live_tx* tx, const void* events, int32_t max_events, int32_t max_bytes,
                               int32_t out_stride, int32_t n_rx_channels, const int32_t* d_channel_map_or_null,
                               int32_t skip_flags, int32_t* out_status, int64_t* out_start, int32_t* out_n_samples,
                               void* hip_stream) {
    return relay_submit(tx, false, events, max_events, max_bytes, out_stride, n_rx_channels, d_channel_map_or_null,
                        skip_flags, nullptr, 0, out_status, out_start, out_n_samples, hip_stream);
}

int afsk_live_tx_submit_events_rated(afsk_live_tx* tx, const void* events, int32_t max_events, int32_t max_bytes,
                                     int32_t out_stride, int32_t n_rx_channels, const int32_t* d_channel_map_or_null,
                                     int32_t skip_flags, const int32_t* d_rx_bit_frames, int32_t rx_slots,
                                     int32_t* out_status, int64_t* out_start, int32_t* out_n_samples,
                                     void* hip_stream) {
    return relay_submit(tx, true, events, max_events, max_bytes, out_stride, n_rx_channels, d_channel_map_or_null,
                        skip_flags, d_rx_bit_frames, rx_slots, out_status, out_start, out_n_samples, hip_stream);
}

}  // extern "C"
