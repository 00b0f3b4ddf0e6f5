// afsk_live_dedup.hip -- the duplicate filter of a live station (afsk_live_dedup_*, afsk_live_tx_submit_events_kept,
// include/afsk_amd.h): a payload a receiver channel has handled within the last `window` samples is not repeated, so two
// relays that hear each other fall silent.  The rule is integer and exact; include/afsk_amd.h states it.
//
// The state is one allocation: DedupEntry [n_channels, depth] ({uint64 key, int64 time}, time INT64_MIN: empty) | int32
// head [n_channels] | 256 bytes of scratch (what the order kernels write); every part 256-byte aligned.
//
// A filter is two launches in order on the caller's stream:
//   live_relay_order_kernel  afsk_live_relay.hip's, unchanged: `stored` and the first unsorted record, written to the
//                            dedup state's own scratch (a transmitter's scratch is not touched).
//   live_dedup_kernel        live_relay_kernel's ownership scheme: one wave per kRelayPerWave record indices, and the wave
//                            that holds the first record of a run of equal channels walks the whole run, so one wave
//                            alone reads and writes a channel's ring -- no atomics, no LDS.  The ring lives in registers
//                            for the run: lane l < depth holds entry l (one 16-byte load).  Per eligible record the 64
//                            lanes add the terms of the payload's bytes (byte loads: inside the payload at any
//                            alignment), a 64-bit butterfly makes the sum and mix64 the key; the lookup is one ballot,
//                            an insertion rewrites lane head's registers, and the lanes whose entry changed store it
//                            when the run ends, lane 0 the head.  Every decision is wave-uniform (a ballot, or a
//                            value read through the first lane); every store is a plain vector store.
// A note is the same two launches over explicit messages: live_tx_order_kernel (afsk_live_tx.hip's, unchanged) over the
// channels and live_dedup_note_kernel, the same wave code reading afsk_live_tx_submit's arrays.
//
// afsk_live_tx_submit_events_kept is afsk_live_tx_submit_events / _rated with a verdict per record: live_relay_kept_kernel
// is live_relay_kernel's text (rated: live_relay_rated_kernel's) with the duplicate check behind the _SKIPPED
// conditions; the two kernels it was copied from keep theirs.
//
// This file is compiled as part of afsk_synth.hip's translation unit (see the #include at its end), behind
// afsk_live_relay.hip, whose order kernel, RelayArgs / RelayRated, vector types and constants it uses.
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace afsk {

constexpr int32_t kDedupMaxDepth = 64;                          // one ring entry per lane
constexpr int64_t kDedupEmpty = INT64_MIN;                      // DedupEntry::time of an empty entry

struct alignas(16) DedupEntry {
    uint64_t key;
    int64_t time;
};
static_assert(sizeof(DedupEntry) == 16, "DedupEntry layout");

struct DedupLayout {
    int64_t n = 0, depth = 0;
    int64_t o_head = 0, o_scratch = 0, bytes = 0;
};

inline int live_dedup_layout(int32_t n_channels, int32_t depth, DedupLayout& L) {
    if (n_channels < 1) return fail(AFSK_E_INVALID_ARG, "afsk_live_dedup: n_channels must be at least 1");
    if (depth < 1 || depth > kDedupMaxDepth) return fail(AFSK_E_INVALID_ARG, "afsk_live_dedup: depth must lie in 1 ... 64");
    L.n = n_channels;
    L.depth = depth;
    L.o_head = tx_align256(16 * L.n * L.depth);
    L.o_scratch = L.o_head + tx_align256(4 * L.n);
    L.bytes = L.o_scratch + 256;
    return AFSK_OK;
}

struct DedupArgs {
    DedupEntry* ring;
    int32_t* head;
    int32_t* verdict;
    int64_t window;
    int32_t count;                  // record places / messages: one verdict each
    int32_t max_bytes;
    int32_t out_stride;             // note: payload_stride
    int32_t n_channels;
    int32_t skip_flags;             // AFSK_LIVE_OVERFLOW included
    int32_t depth;
};

__device__ __forceinline__ uint64_t dedup_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The key of p[0 .. n), the same value in every lane: lane l adds the terms of bytes l, l + 64, ...
__device__ __forceinline__ uint64_t dedup_key(const uint8_t* p, int32_t n, int lane) {
    uint64_t sum = 0;
    for (int32_t i = lane; i < n; i += 64) sum += dedup_mix64(((uint64_t)(uint32_t)i << 8) | p[i]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, s, 64);
    return dedup_mix64(sum ^ ((uint64_t)(uint32_t)n << 32));
}

// One item of a run, as its source reads it: `eligible` items are looked up, the others pass.
struct DedupItem {
    bool eligible;
    const uint8_t* bytes;
    int32_t nbytes;
    int64_t time;
};

// The records of a packed event list (afsk_live_tx_submit_events' reading of them).
struct DedupEventSource {
    const afsk_live_event* records;
    const uint8_t* payload;
    __device__ __forceinline__ int32_t channel(int32_t j) const { return records[j].channel; }
    __device__ __forceinline__ DedupItem item(const DedupArgs& a, int32_t j) const {
        const afsk_live_event r = records[j];
        const int64_t off = r.payload_offset;
        const bool ok = (r.flags & a.skip_flags) == 0 && r.status == AFSK_ST_OK && r.nbytes >= 1 &&
                        r.nbytes <= a.out_stride && off >= 0 && off + r.nbytes <= a.max_bytes;
        return DedupItem{ok, payload + off, r.nbytes,
                         (int64_t)((uint64_t)r.burst_start + (uint64_t)(int64_t)r.burst_len)};
    }
};

// Explicit messages: row j of a [count, payload_stride] matrix, its length and its time.
struct DedupNoteSource {
    const int32_t* channels;
    const uint8_t* payload;
    const int32_t* payload_len;
    const int64_t* time;
    __device__ __forceinline__ int32_t channel(int32_t j) const { return channels[j]; }
    __device__ __forceinline__ DedupItem item(const DedupArgs& a, int32_t j) const {
        const int32_t n = payload_len[j];
        return DedupItem{n >= 1 && n <= a.out_stride, payload + (int64_t)j * a.out_stride, n, time[j]};
    }
};

// What one wave does with its kRelayPerWave indices.  `stored`: items from there on get _NONE; `first_bad`: items from
// there on (below `stored`) get _PASS.
template <class Source>
__device__ __forceinline__ void dedup_wave(const DedupArgs& a, const Source& src, int32_t first_bad, int32_t stored) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = ((int64_t)blockIdx.x * (kRelayThreads / 64) + wave) * kRelayPerWave;
    if (base >= a.count) return;
    auto put = [&](int32_t j, int32_t verdict) {
        if (lane == 0) a.verdict[j] = verdict;
    };
    for (int k = 0; k < kRelayPerWave; k++) {
        const int32_t i = (int32_t)base + k;
        if (i >= a.count) break;
        if (i >= stored) { put(i, AFSK_LIVE_DEDUP_NONE); continue; }
        if (i >= first_bad) { put(i, AFSK_LIVE_DEDUP_PASS); continue; }
        const int32_t ch = src.channel(i);
        if (i > 0 && src.channel(i - 1) == ch) continue;          // not the first of its run
        const bool ok = ch >= 0 && ch < a.n_channels;
        // the channel's ring: entry `lane` in this lane's registers (lanes from depth on hold an empty entry)
        DedupEntry e{0, kDedupEmpty};
        int32_t head = 0;
        if (ok) {
            if (lane < a.depth) e = a.ring[(int64_t)ch * a.depth + lane];
            head = a.head[ch];
            if ((uint32_t)head >= (uint32_t)a.depth) head = 0;    // (afsk_live_dedup_set_state refuses such a head)
        }
        bool mine = false;                                        // this lane's entry was rewritten
        bool inserted = false;
        for (int32_t j = i; j < first_bad && src.channel(j) == ch; j++) {
            const DedupItem it = src.item(a, j);
            if (!ok || !it.eligible) { put(j, AFSK_LIVE_DEDUP_PASS); continue; }
            const uint64_t key = dedup_key(it.bytes, it.nbytes, lane);
            const int64_t t = it.time;
            // 0 <= t - e.time < window without overflow: the age of an entry not in the future fits uint64
            const bool hit = e.time != kDedupEmpty && e.key == key && t >= e.time &&
                             (uint64_t)t - (uint64_t)e.time < (uint64_t)a.window;
            if (__ballot(hit) != 0) { put(j, AFSK_LIVE_DEDUP_DUP); continue; }
            if (lane == head) {
                e = DedupEntry{key, t};
                mine = true;
            }
            head = head + 1 == a.depth ? 0 : head + 1;
            inserted = true;
            put(j, AFSK_LIVE_DEDUP_NEW);
        }
        if (mine) a.ring[(int64_t)ch * a.depth + lane] = e;
        if (inserted && lane == 0) a.head[ch] = head;
    }
}

__global__ __launch_bounds__(kRelayThreads) void live_dedup_kernel(DedupArgs a, const int32_t* __restrict__ scratch,
                                                                   const afsk_live_event* __restrict__ records,
                                                                   const uint8_t* __restrict__ payload) {
    dedup_wave(a, DedupEventSource{records, payload}, scratch[0], scratch[1]);
}

__global__ __launch_bounds__(kRelayThreads) void live_dedup_note_kernel(DedupArgs a, const int32_t* __restrict__ scratch,
                                                                        const int32_t* __restrict__ channels,
                                                                        const uint8_t* __restrict__ payload,
                                                                        const int32_t* __restrict__ payload_len,
                                                                        const int64_t* __restrict__ time) {
    dedup_wave(a, DedupNoteSource{channels, payload, payload_len, time}, scratch[0], a.count);
}

// One thread per ring entry: the masked channels' entries become empty, their heads 0.
__global__ __launch_bounds__(256) void live_dedup_reset_kernel(DedupEntry* ring, int32_t* head,
                                                               const uint8_t* __restrict__ mask, int32_t n_channels,
                                                               int32_t depth) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n_channels * depth) return;
    const int32_t c = (int32_t)(e / depth);
    if (mask && !mask[c]) return;
    ring[e] = DedupEntry{0, kDedupEmpty};
    if (e == (int64_t)c * depth) head[c] = 0;
}

// relay_copy (afsk_live_relay.hip) once more, for the kept kernels alone: a third and fourth caller of relay_copy itself
// changed one instruction of live_relay_rated_kernel (a v_min_i32 became a v_min_u32 in its inlined copy), and the
// kernels this unit had stay as they were, instruction for instruction (profiles/live_dedup_isa.txt).
__device__ __forceinline__ void kept_copy(uint8_t* dst, const uint8_t* src, int32_t len, int lane) {
    const int32_t head = min((int32_t)((16 - ((uintptr_t)dst & 15)) & 15), len);
    if (lane < head) dst[lane] = src[lane];
    const int32_t body = (len - head) >> 4;
    for (int32_t i = lane; i < body; i += 64)
        *reinterpret_cast<relay_vec16*>(dst + head + 16 * (int64_t)i) =
            *reinterpret_cast<const relay_vec16_u*>(src + head + 16 * (int64_t)i);
    const int32_t done = head + 16 * body;
    if (lane < len - done) dst[done + lane] = src[done + lane];
}

// live_relay_kernel (RATED: live_relay_rated_kernel) with a verdict per record: a relayable record whose keep[j] is 0
// answers AFSK_LIVE_TX_DUPLICATE -- behind the _SKIPPED conditions, in front of _BAD_CHANNEL -- and takes no queue slot.
template <bool RATED>
__global__ __launch_bounds__(kRelayThreads) void live_relay_kept_kernel(RelayArgs a, RelayRated rated,
                                                                        const int32_t* __restrict__ scratch,
                                                                        const afsk_live_event* __restrict__ records,
                                                                        const uint8_t* __restrict__ payload,
                                                                        const int32_t* __restrict__ map,
                                                                        const TxGeom* __restrict__ geom,
                                                                        const int32_t* __restrict__ keep) {
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
        TxGeom g = ok && geom ? geom[dst] : TxGeom{a.bf, a.n_train_sym};
        for (int32_t j = i; j < first_bad && records[j].channel == ch; j++) {
            const afsk_live_event r = records[j];
            const int64_t off = r.payload_offset;
            bool skip = (r.flags & a.skip_flags) != 0 || r.status != AFSK_ST_OK || r.nbytes < 1 ||
                        r.nbytes > a.out_stride || off < 0 || off + r.nbytes > a.max_bytes || dropped;
            // (no place in the rate array -- decided before the array is read)
            if (RATED && rated.rx_bf) skip = skip || ch < 0 || ch >= a.n_rx || r.slot < 0 || r.slot >= rated.rx_slots;
            if (skip) { put(j, AFSK_LIVE_TX_SKIPPED, -1, 0); continue; }
            if (keep[j] == 0) { put(j, AFSK_LIVE_TX_DUPLICATE, -1, 0); continue; }
            const int32_t plen = r.nbytes;
            if (!ok) { put(j, AFSK_LIVE_TX_BAD_CHANNEL, -1, 0); continue; }
            if (plen > a.max_payload) { put(j, AFSK_LIVE_TX_TOO_LONG, -1, 0); continue; }
            if (RATED) {
                int32_t idx = 0;                                  // the first table entry at the rate heard
                if (rated.rx_bf) {
                    const int32_t heard = rated.rx_bf[(int64_t)ch * rated.rx_slots + r.slot];
                    while (idx < rated.n_rates && rated.rates[idx].bf != heard) idx++;
                }
                if (idx >= rated.n_rates) { put(j, AFSK_LIVE_TX_BAD_RATE, -1, 0); continue; }
                g = rated.rates[idx];
            }
            if (st.count >= a.depth) { put(j, AFSK_LIVE_TX_QUEUE_FULL, -1, 0); continue; }
            const int64_t start = st.pos > st.end ? st.pos : st.end;
            const int32_t ns = g.bf * (g.n_train_sym + 4 + 14 * plen) + AFSK_TAIL_SILENCE;   // <= AFSK_MAX_STREAM_LEN
            int32_t slot = st.head + st.count;
            if (slot >= a.depth) slot -= a.depth;
            const int64_t e = (int64_t)dst * a.depth + slot;
            if (lane == 0) {
                a.desc[e] = TxDesc{start, ns, plen};
                if (RATED) rated.msg_geom[e] = g;
            }
            kept_copy(a.slots + e * a.max_payload, payload + off, plen, lane);
            st.end = start + ns;
            st.count++;
            put(j, AFSK_LIVE_TX_QUEUED, start, ns);
        }
        if (ok && lane == 0) a.chan[dst] = st;
    }
}

}  // namespace afsk

struct afsk_live_dedup {
    afsk::DeviceState state;                    // DedupLayout::bytes
    afsk::DedupLayout L;
};

namespace {

int dedup_launch_reset(afsk_live_dedup* dd, const uint8_t* mask, hipStream_t st) {
    const afsk::DedupLayout& L = dd->L;
    uint8_t* d = dd->state.ptr();
    hipLaunchKernelGGL(afsk::live_dedup_reset_kernel, dim3((uint32_t)((L.n * L.depth + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<afsk::DedupEntry*>(d), reinterpret_cast<int32_t*>(d + L.o_head), mask,
                       (int32_t)L.n, (int32_t)L.depth);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_dedup_reset_kernel");
}

afsk::DedupArgs dedup_args(afsk_live_dedup* dd, int32_t count, int64_t window, int32_t* d_verdict) {
    const afsk::DedupLayout& L = dd->L;
    uint8_t* d = dd->state.ptr();
    afsk::DedupArgs a{};
    a.ring = reinterpret_cast<afsk::DedupEntry*>(d);
    a.head = reinterpret_cast<int32_t*>(d + L.o_head);
    a.verdict = d_verdict;
    a.window = window;
    a.count = count;
    a.n_channels = (int32_t)L.n;
    a.depth = (int32_t)L.depth;
    return a;
}

uint32_t dedup_blocks(int32_t count) {
    return (uint32_t)(((int64_t)count + afsk::kRelayPerBlock - 1) / afsk::kRelayPerBlock);
}

}  // namespace

extern "C" {

int afsk_live_dedup_layout(int32_t n_channels, int32_t depth, int64_t* out_state_bytes) {
    afsk::DedupLayout L;
    if (int rc = afsk::live_dedup_layout(n_channels, depth, L)) return rc;
    if (out_state_bytes) *out_state_bytes = L.bytes;
    return AFSK_OK;
}

int afsk_live_dedup_create(int32_t n_channels, int32_t depth, afsk_live_dedup** out) {
    if (!out) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_create: null pointer argument");
    *out = nullptr;
    return afsk::no_throw([&] {
        std::unique_ptr<afsk_live_dedup> dd(new afsk_live_dedup());
        if (int rc = afsk::live_dedup_layout(n_channels, depth, dd->L)) return rc;
        // the heads and the scratch are zeroed; the entries are emptied by the reset kernel (an empty time is not 0)
        if (int rc = dd->state.create("afsk_live_dedup_create", dd->L.bytes, dd->L.bytes)) return rc;
        if (int rc = dedup_launch_reset(dd.get(), nullptr, nullptr)) return rc;
        hipError_t e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return afsk::hip_fail(e, "afsk_live_dedup_create (empty the rings)");
        *out = dd.release();
        return (int)AFSK_OK;
    });
}

int afsk_live_dedup_destroy(afsk_live_dedup* dd) {
    delete dd;        // the caller has synchronised the launches that use it
    return AFSK_OK;
}

int afsk_live_dedup_reset(afsk_live_dedup* dd, const uint8_t* d_mask_or_null, void* hip_stream) {
    if (!dd) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_reset: null duplicate filter");
    if (int rc = dd->state.check_current()) return rc;
    return dedup_launch_reset(dd, d_mask_or_null, (hipStream_t)hip_stream);
}

int afsk_live_dedup_get_state(afsk_live_dedup* dd, void* host_out, int64_t bytes) {
    if (!dd || !host_out) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_get_state: null pointer argument");
    if (bytes != dd->L.o_scratch)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_get_state: bytes must be the state's without its scratch "
                                              "(afsk_live_dedup_layout's - 256)");
    if (int rc = dd->state.check_current()) return rc;
    hipError_t e = hipMemcpy(host_out, dd->state.d, (size_t)bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "afsk_live_dedup_get_state (hipMemcpy)");
}

int afsk_live_dedup_set_state(afsk_live_dedup* dd, const void* host_in, int64_t bytes) {
    if (!dd || !host_in) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_set_state: null pointer argument");
    if (bytes != dd->L.o_scratch)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_set_state: bytes must be the state's without its scratch "
                                              "(afsk_live_dedup_layout's - 256)");
    const int32_t* head = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(host_in) + dd->L.o_head);
    for (int64_t c = 0; c < dd->L.n; c++)
        if (head[c] < 0 || head[c] >= dd->L.depth)
            return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_set_state: the head of channel " + std::to_string(c) +
                                                      " lies outside 0 ... depth - 1");
    if (int rc = dd->state.check_current()) return rc;
    hipError_t e = hipMemcpy(dd->state.d, host_in, (size_t)bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "afsk_live_dedup_set_state (hipMemcpy)");
}

int afsk_live_dedup_filter(afsk_live_dedup* dd, const void* events, int32_t max_events, int32_t max_bytes,
                           int32_t out_stride, int32_t skip_flags, int64_t window, int32_t* d_verdict,
                           void* hip_stream) {
    if (!dd) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_filter: null duplicate filter");
    if (max_events < 0 || max_bytes < 0 || out_stride < 0)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_filter: negative size");
    if (window < 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_filter: negative window");
    if (skip_flags & ~(AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW))
        return afsk::fail(AFSK_E_INVALID_ARG,
                          "afsk_live_dedup_filter: skip_flags may hold AFSK_LIVE_OPEN_END and AFSK_LIVE_OVERFLOW alone");
    if (!events || !d_verdict) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_filter: null pointer argument");
    if ((uintptr_t)events & 15)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_filter: the events buffer must be 16-byte aligned");
    if (max_events == 0) return AFSK_OK;
    if (int rc = dd->state.check_current()) return rc;
    const uint8_t* ev = static_cast<const uint8_t*>(events);
    const afsk_live_event* records = reinterpret_cast<const afsk_live_event*>(ev + afsk::kRelayHeaderBytes);
    const uint8_t* payload = ev + afsk::kRelayHeaderBytes + (int64_t)sizeof(afsk_live_event) * max_events;
    int32_t* scratch = reinterpret_cast<int32_t*>(dd->state.ptr() + dd->L.o_scratch);
    afsk::DedupArgs a = dedup_args(dd, max_events, window, d_verdict);
    a.max_bytes = max_bytes;
    a.out_stride = out_stride;
    a.skip_flags = skip_flags | AFSK_LIVE_OVERFLOW;
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_relay_order_kernel, dim3(1), dim3(afsk::kOrderThreads), 0, st,
                       reinterpret_cast<const int32_t*>(ev) /* the header: [1] is `stored` */, records, max_events,
                       scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_relay_order_kernel");
    hipLaunchKernelGGL(afsk::live_dedup_kernel, dim3(dedup_blocks(max_events)), dim3(afsk::kRelayThreads), 0, st, a,
                       (const int32_t*)scratch, records, payload);
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_dedup_kernel");
}

int afsk_live_dedup_note(afsk_live_dedup* dd, const int32_t* d_channels, const uint8_t* d_payload,
                         int32_t payload_stride, const int32_t* d_payload_len, const int64_t* d_time,
                         int32_t n_messages, int64_t window, int32_t* d_verdict, void* hip_stream) {
    if (!dd) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_note: null duplicate filter");
    if (n_messages < 0 || payload_stride < 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_note: negative size");
    if (window < 0) return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_note: negative window");
    if (n_messages == 0) return AFSK_OK;
    if (!d_channels || !d_payload || !d_payload_len || !d_time || !d_verdict)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_dedup_note: null pointer argument");
    if (int rc = dd->state.check_current()) return rc;
    int32_t* scratch = reinterpret_cast<int32_t*>(dd->state.ptr() + dd->L.o_scratch);
    afsk::DedupArgs a = dedup_args(dd, n_messages, window, d_verdict);
    a.out_stride = payload_stride;
    const hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(afsk::live_tx_order_kernel, dim3(1), dim3(256), 0, st, d_channels, n_messages, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_tx_order_kernel");
    hipLaunchKernelGGL(afsk::live_dedup_note_kernel, dim3(dedup_blocks(n_messages)), dim3(afsk::kRelayThreads), 0, st, a,
                       (const int32_t*)scratch, d_channels, d_payload, d_payload_len, d_time);
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_dedup_note_kernel");
}

int afsk_live_tx_submit_events_kept(afsk_live_tx* tx, const void* events, int32_t max_events, int32_t max_bytes,
                                    int32_t out_stride, int32_t n_rx_channels, const int32_t* d_channel_map_or_null,
                                    int32_t skip_flags, const int32_t* d_rx_bit_frames_or_null, int32_t rx_slots,
                                    const int32_t* d_keep, int32_t* out_status, int64_t* out_start,
                                    int32_t* out_n_samples, void* hip_stream) {
    const char* who = "afsk_live_tx_submit_events_kept: ";
    if (!tx) return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "null live transmitter");
    if (max_events < 0 || max_bytes < 0 || out_stride < 0)
        return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "negative size");
    if (n_rx_channels < 1) return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "n_rx_channels must be at least 1");
    if (skip_flags & ~(AFSK_LIVE_OPEN_END | AFSK_LIVE_OVERFLOW))
        return afsk::fail(AFSK_E_INVALID_ARG,
                          std::string(who) + "skip_flags may hold AFSK_LIVE_OPEN_END and AFSK_LIVE_OVERFLOW alone");
    if (!events || !d_keep || !out_status || !out_start || !out_n_samples)
        return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "null pointer argument");
    if (d_rx_bit_frames_or_null && rx_slots < 1)
        return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "rx_slots must be at least 1 with d_rx_bit_frames");
    if (d_rx_bit_frames_or_null && tx->n_rates == 0)
        return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "d_rx_bit_frames needs a transmitter of "
                                                                 "afsk_live_tx_create_rated (pass NULL to this one)");
    if ((uintptr_t)events & 15)
        return afsk::fail(AFSK_E_INVALID_ARG, std::string(who) + "the events buffer must be 16-byte aligned");
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
    const afsk_live_event* records = reinterpret_cast<const afsk_live_event*>(ev + afsk::kRelayHeaderBytes);
    const uint8_t* payload = ev + afsk::kRelayHeaderBytes + (int64_t)sizeof(afsk_live_event) * max_events;
    const afsk::TxGeom* geom = tx->o_geom ? reinterpret_cast<const afsk::TxGeom*>(d + tx->o_geom) : nullptr;
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
                       reinterpret_cast<const int32_t*>(ev) /* the header: [1] is `stored` */, records, max_events,
                       scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return afsk::hip_fail(e, "launch live_relay_order_kernel");
    afsk::RelayRated rated{};
    if (tx->n_rates) {
        rated.rates = reinterpret_cast<const afsk::TxGeom*>(d + tx->R.o_rates);
        rated.msg_geom = reinterpret_cast<afsk::TxGeom*>(d + tx->R.o_msg_geom);
        rated.rx_bf = d_rx_bit_frames_or_null;
        rated.n_rates = tx->n_rates;
        rated.rx_slots = rx_slots;
        hipLaunchKernelGGL(afsk::live_relay_kept_kernel<true>, dim3(dedup_blocks(max_events)),
                           dim3(afsk::kRelayThreads), 0, st, a, rated, (const int32_t*)scratch, records, payload,
                           d_channel_map_or_null, geom, d_keep);
    } else {
        hipLaunchKernelGGL(afsk::live_relay_kept_kernel<false>, dim3(dedup_blocks(max_events)),
                           dim3(afsk::kRelayThreads), 0, st, a, rated, (const int32_t*)scratch, records, payload,
                           d_channel_map_or_null, geom, d_keep);
    }
    e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch live_relay_kept_kernel");
}

}  // extern "C"
