// afsk_live_events.hip -- the packed event list of a live push (afsk_live_events_layout / afsk_live_pack,
// include/afsk_amd.h): the slot-indexed outputs of one push -- n_closed, the gate's three slot arrays, the demodulator's
// five vectors and its payload rows -- turned into a count, that many fixed-size records and the payload bytes back to
// back, so that the host copies in proportion to what closed, not to n_channels * slots.
//
// The events buffer (one caller-provided allocation, 16-byte aligned):
//   [0, 32)                       LiveEventsHeader
//   [32, 32 + 48 * max_events)    afsk_live_event records, channel ascending, then slot ascending
//   [payload_offset, + max_bytes) the records' kept payload bytes back to back in record order
//   [scratch_offset, total)       one LiveEventsTotal (16 bytes) per span of kLiveEventsSpan channels
//
// Three ordinary launches in order on the caller's stream, a thread per channel, kLiveEventsSpan channels per block:
//   live_events_total_kernel  block b sums the bursts and the kept payload bytes of its span into scratch[b]
//   live_events_scan_kernel   ONE block walks scratch front to back, 256 entries per step, and replaces every entry by
//                             the sums of the entries before it; then it writes the header
//   live_events_write_kernel  block b scans its span (wave scans, the waves' totals through LDS), starts at scratch[b]
//                             and writes its records and payloads, a wave per record
// No block ever waits for another: the order of the launches is the only dependency, and the work is linear in
// n_channels (n_channels reads of n_closed in the first and the third launch, n_channels / 256 entries in the second).
// The slot arrays and payload rows are read only for slots k < n_closed[c].
//
// stored_bytes: the kept bytes of record r start at off_r, the sum of the kept bytes before it, and are written when
// r < max_events and off_r + kept_r <= max_bytes; off_r never decreases, so the written payloads are those of the first
// W records and stored_bytes = off_W.  The scan kernel writes the header with stored_bytes = n_bytes (W = count); when
// W < count, record W is found by its own values alone -- it is record max_events with off <= max_bytes, or a record
// below max_events with off <= max_bytes < off + kept -- and the wave that holds it overwrites stored_bytes with off.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end).

namespace afsk {

constexpr int kLiveEventsSpan = 256;        // channels per block = threads per block: AFSK_LIVE_EVENTS_SPAN

struct LiveEventsHeader {
    int32_t count;
    int32_t stored;
    int64_t n_bytes;
    int64_t stored_bytes;
    int64_t reserved;
};
static_assert(sizeof(LiveEventsHeader) == 32, "the events header is 32 bytes");
static_assert(sizeof(afsk_live_event) == 48 && offsetof(afsk_live_event, burst_start) == 8 &&
                  offsetof(afsk_live_event, burst_len) == 16 && offsetof(afsk_live_event, payload_offset) == 44,
              "afsk_live_event is 48 bytes without padding");

// the bursts and kept payload bytes of a span (first launch), then of all spans before it (second launch)
struct LiveEventsTotal {
    int64_t events;
    int64_t bytes;
};

struct LiveEventsLayout {
    int64_t o_records, o_payload, o_scratch, total, blocks;
};

struct LiveEventsArgs {
    int32_t n, slots;
    const int32_t* n_closed;
    const int64_t* burst_start;
    const int32_t* burst_len;
    const int32_t* flags;
    const uint8_t* out_bytes;
    int32_t out_stride;
    const int32_t* nbytes;
    const int32_t* nbits;
    const int32_t* clock_idx;
    const int32_t* term_frame;
    const int32_t* status;
    LiveEventsHeader* header;
    afsk_live_event* records;
    uint8_t* payload;
    LiveEventsTotal* scratch;
    int32_t max_events;
    int64_t max_bytes;
    int64_t blocks;
};

typedef uint32_t ev_vec16 __attribute__((ext_vector_type(4)));
typedef uint32_t ev_vec16_u __attribute__((ext_vector_type(4), aligned(1)));     // a payload row starts at any byte

// the payload bytes a record keeps: min(max(nbytes, 0), out_stride), none for an overflowed burst
__device__ __forceinline__ int32_t live_event_kept(int32_t nbytes, int32_t flags, int32_t out_stride) {
    return (flags & AFSK_LIVE_OVERFLOW) ? 0 : min(max(nbytes, 0), out_stride);
}

// (bursts, kept bytes) of channel c: reads the slots in use only
__device__ __forceinline__ void live_events_channel(const LiveEventsArgs& a, int c, int32_t& e, int64_t& kb) {
    e = 0;
    kb = 0;
    if (c >= a.n) return;
    e = min(max(a.n_closed[c], 0), a.slots);
    const int64_t row = (int64_t)c * a.slots;
    for (int k = 0; k < e; k++) kb += live_event_kept(a.nbytes[row + k], a.flags[row + k], a.out_stride);
}

// inclusive scan over the wave (lane l: the sum of lanes 0 ... l)
__device__ __forceinline__ void live_events_wave_scan(int32_t& e, int64_t& kb, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t pe = __shfl_up(e, d);
        const int64_t pb = __shfl_up(kb, d);
        if (lane >= d) {
            e += pe;
            kb += pb;
        }
    }
}

// inclusive scan over the block's 256 threads; returns the block's totals in te / tb
__device__ __forceinline__ void live_events_block_scan(int32_t& e, int64_t& kb, int32_t& te, int64_t& tb) {
    __shared__ int32_t s_e[4];
    __shared__ int64_t s_b[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    live_events_wave_scan(e, kb, lane);
    __syncthreads();                                    // (the previous use of s_e / s_b has been read)
    if (lane == 63) {
        s_e[w] = e;
        s_b[w] = kb;
    }
    __syncthreads();
    te = 0;
    tb = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (j < w) {
            e += s_e[j];
            kb += s_b[j];
        }
        te += s_e[j];
        tb += s_b[j];
    }
}

__global__ __launch_bounds__(kLiveEventsSpan) void live_events_total_kernel(LiveEventsArgs a) {
    const int64_t c = (int64_t)blockIdx.x * kLiveEventsSpan + threadIdx.x;
    int32_t e, te;
    int64_t kb, tb;
    live_events_channel(a, c < a.n ? (int)c : a.n, e, kb);
    live_events_block_scan(e, kb, te, tb);
    if (threadIdx.x == 0) a.scratch[blockIdx.x] = LiveEventsTotal{te, tb};
}

__global__ __launch_bounds__(kLiveEventsSpan) void live_events_scan_kernel(LiveEventsArgs a) {
    int64_t carry_e = 0, carry_b = 0;
    for (int64_t base = 0; base < a.blocks; base += kLiveEventsSpan) {
        const int64_t i = base + threadIdx.x;
        LiveEventsTotal t{0, 0};
        if (i < a.blocks) t = a.scratch[i];
        int32_t e = (int32_t)t.events, te;              // (a span holds at most 256 * slots < 2^31 bursts)
        int64_t kb = t.bytes, tb;
        live_events_block_scan(e, kb, te, tb);
        if (i < a.blocks) a.scratch[i] = LiveEventsTotal{carry_e + e - t.events, carry_b + kb - t.bytes};
        carry_e += te;
        carry_b += tb;
    }
    if (threadIdx.x == 0) {
        LiveEventsHeader h;
        h.count = (int32_t)carry_e;                     // <= n_channels * slots < 2^31
        h.stored = (int32_t)(carry_e < a.max_events ? carry_e : a.max_events);
        h.n_bytes = carry_b;
        h.stored_bytes = carry_b;                       // (the write kernel corrects it when a payload is left out)
        h.reserved = 0;
        *a.header = h;
    }
}

// kept bytes from src to dst, by the whole wave: bytes up to dst's next 16-byte boundary, 16-byte stores, bytes
__device__ __forceinline__ void live_events_copy(uint8_t* dst, const uint8_t* src, int32_t kept, int lane) {
    const int32_t head = min((int32_t)((16 - ((uintptr_t)dst & 15)) & 15), kept);
    if (lane < head) dst[lane] = src[lane];
    const int32_t body = (kept - head) >> 4;
    for (int32_t i = lane; i < body; i += 64)
        *reinterpret_cast<ev_vec16*>(dst + head + 16 * (int64_t)i) =
            *reinterpret_cast<const ev_vec16_u*>(src + head + 16 * (int64_t)i);
    const int32_t done = head + 16 * body;
    if (lane < kept - done) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(kLiveEventsSpan) void live_events_write_kernel(LiveEventsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t cc = (int64_t)blockIdx.x * kLiveEventsSpan + threadIdx.x;
    const int c = cc < a.n ? (int)cc : a.n;
    int32_t e, te;
    int64_t kb, tb;
    live_events_channel(a, c, e, kb);
    int32_t ie = e;
    int64_t ib = kb;
    live_events_block_scan(ie, ib, te, tb);
    if (te == 0) return;                                // (uniform over the block)
    const LiveEventsTotal before = a.scratch[blockIdx.x];
    const int64_t first = before.events + ie - e;       // the index of this channel's first record
    const int64_t off0 = before.bytes + ib - kb;        // and where its payload starts
    // the wave takes its channels that reported bursts one after the other, and every record of a channel as one
    uint64_t todo = __ballot(e > 0);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int ch = __shfl(c, src);
        const int32_t ne = __shfl(e, src);
        int64_t idx = __shfl(first, src);
        int64_t off = __shfl(off0, src);
        const int64_t row = (int64_t)ch * a.slots;
        for (int k = 0; k < ne; k++, idx++) {
            const int32_t nb = a.nbytes[row + k], fl = a.flags[row + k];
            const int32_t kept = live_event_kept(nb, fl, a.out_stride);
            const bool fits = off + kept <= a.max_bytes;
            if (idx < a.max_events) {
                if (lane == 0) {
                    afsk_live_event r;
                    r.channel = ch;
                    r.slot = k;
                    r.burst_start = a.burst_start[row + k];
                    r.burst_len = a.burst_len[row + k];
                    r.flags = fl;
                    r.status = a.status[row + k];
                    r.nbytes = nb;
                    r.nbits = a.nbits[row + k];
                    r.clock_idx = a.clock_idx[row + k];
                    r.term_frame = a.term_frame[row + k];
                    r.payload_offset = fits ? (int32_t)off : -1;
                    a.records[idx] = r;
                    if (!fits && off <= a.max_bytes) a.header->stored_bytes = off;      // the first payload left out
                }
                if (fits && kept > 0)
                    live_events_copy(a.payload + off, a.out_bytes + (row + k) * a.out_stride, kept, lane);
            } else if (idx == a.max_events && off <= a.max_bytes && lane == 0) {
                a.header->stored_bytes = off;                                            // the first record left out
            }
            off += kept;
        }
    }
}

// AFSK_E_INVALID_ARG unless the sizes are those afsk_live_events_layout accepts; the layout in L
inline int live_events_layout(int32_t n_channels, int32_t slots, int32_t max_events, int64_t max_bytes,
                              LiveEventsLayout& L) {
    if (n_channels < 1 || slots < 1) return fail(AFSK_E_INVALID_ARG, "n_channels and slots must be at least 1");
    if ((int64_t)n_channels * slots >= (1ll << 31))
        return fail(AFSK_E_INVALID_ARG, "n_channels * slots must stay below 2^31");
    if (max_events < 0 || max_bytes < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (max_bytes >= (1ll << 31)) return fail(AFSK_E_INVALID_ARG, "max_bytes must stay below 2^31");
    L.blocks = AFSK_LIVE_EVENTS_BLOCKS(n_channels);
    L.o_records = (int64_t)sizeof(LiveEventsHeader);
    L.o_payload = L.o_records + (int64_t)sizeof(afsk_live_event) * max_events;
    L.o_scratch = (L.o_payload + max_bytes + 15) & ~15ll;
    L.total = L.o_scratch + (int64_t)sizeof(LiveEventsTotal) * L.blocks;
    return AFSK_OK;
}

}  // namespace afsk

extern "C" {

int afsk_live_events_layout(int32_t n_channels, int32_t slots, int32_t max_events, int64_t max_bytes,
                            int64_t* out_records_offset, int64_t* out_payload_offset, int64_t* out_total_bytes) {
    afsk::LiveEventsLayout L;
    if (int rc = afsk::live_events_layout(n_channels, slots, max_events, max_bytes, L)) return rc;
    if (!out_records_offset || !out_payload_offset || !out_total_bytes)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out_records_offset = L.o_records;
    *out_payload_offset = L.o_payload;
    *out_total_bytes = L.total;
    return AFSK_OK;
}

int afsk_live_pack(int32_t n_channels, int32_t slots, const int32_t* n_closed, const int64_t* burst_start,
                   const int32_t* burst_len, const int32_t* flags, const uint8_t* out_bytes, int32_t out_stride,
                   const int32_t* nbytes, const int32_t* nbits, const int32_t* clock_idx, const int32_t* term_frame,
                   const int32_t* status, void* events, int32_t max_events, int64_t max_bytes, void* hip_stream) {
    using namespace afsk;
    LiveEventsLayout L;
    if (int rc = live_events_layout(n_channels, slots, max_events, max_bytes, L)) return rc;
    if (out_stride < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (!n_closed || !burst_start || !burst_len || !flags || (!out_bytes && out_stride != 0) || !nbytes || !nbits ||
        !clock_idx || !term_frame || !status || !events)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if ((uintptr_t)events & 15) return fail(AFSK_E_INVALID_ARG, "the events buffer must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    uint8_t* ev = static_cast<uint8_t*>(events);
    const LiveEventsArgs a{n_channels, slots, n_closed, burst_start, burst_len, flags, out_bytes, out_stride,
                           nbytes, nbits, clock_idx, term_frame, status,
                           reinterpret_cast<LiveEventsHeader*>(ev),
                           reinterpret_cast<afsk_live_event*>(ev + L.o_records), ev + L.o_payload,
                           reinterpret_cast<LiveEventsTotal*>(ev + L.o_scratch), max_events, max_bytes, L.blocks};
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid((uint32_t)L.blocks), block(kLiveEventsSpan);
    hipLaunchKernelGGL(live_events_total_kernel, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_events_total_kernel");
    hipLaunchKernelGGL(live_events_scan_kernel, dim3(1), block, 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_events_scan_kernel");
    hipLaunchKernelGGL(live_events_write_kernel, grid, block, 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_events_write_kernel");
    return AFSK_OK;
}

}  // extern "C"
