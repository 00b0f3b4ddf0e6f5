// afsk_live_pack.hip -- the two packed lists of a live push (include/afsk_amd.h), each a count, that many fixed-size
// records and their bytes back to back in one buffer, so that the host copies in proportion to what happened, not to
// the size of the per-channel arrays:
//   events    afsk_live_events_layout / afsk_live_pack: the slot-indexed outputs of one push -- n_closed, the gate's
//             three slot arrays, the demodulator's five vectors and its payload rows -- as one afsk_live_event per
//             reported burst and the kept payload bytes
//   segments  afsk_live_segments_layout / afsk_live_pack_tap: what the payload tap of a progressive push handed out --
//             per channel the shares of the bursts it reported and the share of the burst still recording -- as one
//             afsk_live_segment per share and the tap bytes
//
// A packed buffer (one caller-provided allocation, 16-byte aligned; R = sizeof the record, 48 or 32):
//   [0, 32)                        LivePackHeader
//   [32, 32 + R * max_records)     the records: channel ascending, then slot ascending (then the open segment)
//   [bytes_offset, + max_bytes)    the records' kept bytes back to back in record order
//   [scratch_offset, total)        one LivePackTotal (16 bytes) per span of kLivePackSpan channels
//
// A pack is three ordinary launches in order on the caller's stream (live_pack_launch), a thread per channel,
// kLivePackSpan channels per block:
//   live_pack_total_kernel<Args>   block b sums the records and the kept bytes of its span into scratch[b]
//   live_pack_scan_kernel          ONE block walks scratch front to back, 256 entries per step, and replaces every entry
//                                  by the sums of the entries before it; then it writes the header
//   live_events_write_kernel /     block b scans its span (wave scans, the waves' totals through LDS), starts at
//   live_segments_write_kernel     scratch[b] and writes its records and bytes
// No block ever waits for another: the order of the launches is the only dependency, and the work is linear in
// n_channels (n_channels reads of n_closed in the first and the third launch, n_channels / 256 entries in the second).
//
// What is shared is everything that does not look at a record: the header, the totals, the scans, the layout, the
// first two kernels and the launches.  A packer adds its inputs (LiveEventsArgs / LiveSegmentsArgs, each ending in the
// same LivePackOut), its per-channel rule (live_pack_count) and its write kernel.  The write kernels differ on purpose:
// a burst closes on few channels and carries a payload row, so the events are written a wave per record (the wave
// copies the row with 16-byte stores); a list of segments is dense whenever the channels are busy -- an open gate gives
// a segment in every push -- so the segments are written a thread per channel: 64 channels of a wave side by side,
// where a wave per channel would take them in 64 rounds of about 14 bytes.
//
// stored_bytes: the kept bytes of record r start at off_r, the sum of the kept bytes before it, and are written when
// r < max_records and off_r + kept_r <= max_bytes; off_r never decreases, so the written ones are those of the first
// W records and stored_bytes = off_W.  The scan kernel writes the header with stored_bytes = n_bytes (W = count); when
// W < count, record W is found by its own values alone -- it is record max_records with off <= max_bytes, or a record
// below max_records with off <= max_bytes < off + kept -- and the wave / thread that holds it overwrites stored_bytes.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end).

namespace afsk {

constexpr int kLivePackSpan = AFSK_LIVE_EVENTS_SPAN;    // channels per block = threads per block

struct LivePackHeader {
    int32_t count;
    int32_t stored;
    int64_t n_bytes;
    int64_t stored_bytes;
    int64_t reserved;
};
static_assert(sizeof(LivePackHeader) == 32, "the header of a packed list is 32 bytes");
static_assert(sizeof(afsk_live_event) == 48 && offsetof(afsk_live_event, burst_start) == 8 &&
                  offsetof(afsk_live_event, burst_len) == 16 && offsetof(afsk_live_event, payload_offset) == 44,
              "afsk_live_event is 48 bytes without padding");
static_assert(sizeof(afsk_live_segment) == 32 && offsetof(afsk_live_segment, burst_start) == 8 &&
                  offsetof(afsk_live_segment, burst_len) == 16 && offsetof(afsk_live_segment, length) == 28,
              "afsk_live_segment is 32 bytes without padding");

// the records and kept bytes of a span (first launch), then of all spans before it (second launch)
struct LivePackTotal {
    int64_t records;
    int64_t bytes;
};

struct LivePackLayout {
    int64_t o_records, o_bytes, o_scratch, total, blocks;
};

// where a pack writes: the last member of a packer's arguments
template <typename Record>
struct LivePackOut {
    LivePackHeader* header;
    Record* records;
    uint8_t* bytes;
    LivePackTotal* scratch;
    int32_t max_records;
    int64_t max_bytes;
    int64_t blocks;
};

// what of it the scan kernel needs
struct LivePackScanArgs {
    LivePackHeader* header;
    LivePackTotal* scratch;
    int32_t max_records;
    int64_t blocks;
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
    LivePackOut<afsk_live_event> out;
};

struct LiveSegmentsArgs {
    int32_t n, slots, tap_cap;
    const int32_t* n_closed;
    const int64_t* burst_start;
    const int32_t* burst_len;
    const int32_t* flags;
    const int32_t* nbytes;
    const uint8_t* tap_bytes;
    const int32_t* tap_n;
    const int32_t* tap_len;
    const int64_t* open_start;
    const int32_t* open_nbytes;
    LivePackOut<afsk_live_segment> out;
};

typedef uint32_t ev_vec16 __attribute__((ext_vector_type(4)));
typedef uint32_t ev_vec16_u __attribute__((ext_vector_type(4), aligned(1)));     // a payload row starts at any byte

// ---- the per-channel rules ----

// the payload bytes an event keeps: min(max(nbytes, 0), out_stride), none for an overflowed burst
__device__ __forceinline__ int32_t live_event_kept(int32_t nbytes, int32_t flags, int32_t out_stride) {
    return (flags & AFSK_LIVE_OVERFLOW) ? 0 : min(max(nbytes, 0), out_stride);
}

// (bursts, kept bytes) of channel c: reads the slots in use only (slots k < n_closed[c])
__device__ __forceinline__ void live_events_channel(const LiveEventsArgs& a, int c, int32_t& e, int64_t& kb) {
    e = 0;
    kb = 0;
    if (c >= a.n) return;
    e = min(max(a.n_closed[c], 0), a.slots);
    const int64_t row = (int64_t)c * a.slots;
    for (int k = 0; k < e; k++) kb += live_event_kept(a.nbytes[row + k], a.flags[row + k], a.out_stride);
}

// The segments of channel c: nc = clamp(n_closed[c], 0, slots), tn = clamp(tap_n[c], 0, tap_cap); slot k < nc takes
// ln_k = clamp(tap_len[c, k], 0, tn - at) bytes of the tap row from at on, at += ln_k; rest = tn - at is the open
// segment's when rest > 0 and open_start[c] >= 0.  nc final records (length 0 where a burst closed without new bytes),
// then the open one; their bytes are ONE run of the tap row and land as one run of the bytes part.  (records, bytes) in
// e / kb.  Reads n_closed and tap_n, tap_len for k < nc, open_start where rest > 0.
__device__ __forceinline__ void live_segments_channel(const LiveSegmentsArgs& a, int c, int32_t& nc, int32_t& tn,
                                                      int32_t& at, bool& open, int32_t& e, int64_t& kb) {
    nc = tn = at = e = 0;
    open = false;
    kb = 0;
    if (c >= a.n) return;
    nc = min(max(a.n_closed[c], 0), a.slots);
    tn = min(max(a.tap_n[c], 0), a.tap_cap);
    const int64_t row = (int64_t)c * a.slots;
    for (int k = 0; k < nc; k++) at += min(max(a.tap_len[row + k], 0), tn - at);
    open = tn > at && a.open_start[c] >= 0;
    e = nc + (open ? 1 : 0);
    kb = open ? tn : at;
}

// (records, kept bytes) of channel c, per packer: what the total kernel sums
__device__ __forceinline__ void live_pack_count(const LiveEventsArgs& a, int c, int32_t& e, int64_t& kb) {
    live_events_channel(a, c, e, kb);
}
__device__ __forceinline__ void live_pack_count(const LiveSegmentsArgs& a, int c, int32_t& e, int64_t& kb) {
    int32_t nc, tn, at;
    bool open;
    live_segments_channel(a, c, nc, tn, at, open, e, kb);
}

// ---- the shared part: scans, the first two kernels, the layout, the launches ----

// inclusive scan over the wave (lane l: the sum of lanes 0 ... l)
__device__ __forceinline__ void live_pack_wave_scan(int32_t& e, int64_t& kb, int lane) {
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
__device__ __forceinline__ void live_pack_block_scan(int32_t& e, int64_t& kb, int32_t& te, int64_t& tb) {
    __shared__ int32_t s_e[4];
    __shared__ int64_t s_b[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    live_pack_wave_scan(e, kb, lane);
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

template <typename Args>
__global__ __launch_bounds__(kLivePackSpan) void live_pack_total_kernel(Args a) {
    const int64_t c = (int64_t)blockIdx.x * kLivePackSpan + threadIdx.x;
    int32_t e, te;
    int64_t kb, tb;
    live_pack_count(a, c < a.n ? (int)c : a.n, e, kb);
    live_pack_block_scan(e, kb, te, tb);
    if (threadIdx.x == 0) a.out.scratch[blockIdx.x] = LivePackTotal{te, tb};
}

__global__ __launch_bounds__(kLivePackSpan) void live_pack_scan_kernel(LivePackScanArgs a) {
    int64_t carry_e = 0, carry_b = 0;
    for (int64_t base = 0; base < a.blocks; base += kLivePackSpan) {
        const int64_t i = base + threadIdx.x;
        LivePackTotal t{0, 0};
        if (i < a.blocks) t = a.scratch[i];
        int32_t e = (int32_t)t.records, te;             // (a span holds at most 256 * (slots + 1) < 2^31 records)
        int64_t kb = t.bytes, tb;
        live_pack_block_scan(e, kb, te, tb);
        if (i < a.blocks) a.scratch[i] = LivePackTotal{carry_e + e - t.records, carry_b + kb - t.bytes};
        carry_e += te;
        carry_b += tb;
    }
    if (threadIdx.x == 0) {
        LivePackHeader h;
        // saturates: n_channels * (slots + 1) segments may pass 2^31 - 1; n_channels * slots events cannot
        h.count = (int32_t)(carry_e < 0x7fffffffll ? carry_e : 0x7fffffffll);
        h.stored = (int32_t)(carry_e < a.max_records ? carry_e : a.max_records);
        h.n_bytes = carry_b;
        h.stored_bytes = carry_b;                       // (the write kernel corrects it when bytes are left out)
        h.reserved = 0;
        *a.header = h;
    }
}

// AFSK_E_INVALID_ARG unless the sizes are those the layout entries accept; the layout for records of record_size in L
inline int live_pack_layout(int32_t n_channels, int32_t slots, int64_t record_size, int32_t max_records,
                            int64_t max_bytes, LivePackLayout& L) {
    if (n_channels < 1 || slots < 1) return fail(AFSK_E_INVALID_ARG, "n_channels and slots must be at least 1");
    if ((int64_t)n_channels * slots >= (1ll << 31))
        return fail(AFSK_E_INVALID_ARG, "n_channels * slots must stay below 2^31");
    if (max_records < 0 || max_bytes < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (max_bytes >= (1ll << 31)) return fail(AFSK_E_INVALID_ARG, "max_bytes must stay below 2^31");
    L.blocks = AFSK_LIVE_EVENTS_BLOCKS(n_channels);
    L.o_records = (int64_t)sizeof(LivePackHeader);
    L.o_bytes = L.o_records + record_size * max_records;
    L.o_scratch = (L.o_bytes + max_bytes + 15) & ~15ll;
    L.total = L.o_scratch + (int64_t)sizeof(LivePackTotal) * L.blocks;
    return AFSK_OK;
}

// the two layout entries
inline int live_pack_layout_entry(int32_t n_channels, int32_t slots, int64_t record_size, int32_t max_records,
                                  int64_t max_bytes, int64_t* out_records_offset, int64_t* out_bytes_offset,
                                  int64_t* out_total_bytes) {
    LivePackLayout L;
    if (int rc = live_pack_layout(n_channels, slots, record_size, max_records, max_bytes, L)) return rc;
    if (!out_records_offset || !out_bytes_offset || !out_total_bytes)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out_records_offset = L.o_records;
    *out_bytes_offset = L.o_bytes;
    *out_total_bytes = L.total;
    return AFSK_OK;
}

// the parts of `buffer` (laid out as L) a pack writes
template <typename Record>
LivePackOut<Record> live_pack_out(void* buffer, const LivePackLayout& L, int32_t max_records, int64_t max_bytes) {
    uint8_t* b = static_cast<uint8_t*>(buffer);
    return {reinterpret_cast<LivePackHeader*>(b), reinterpret_cast<Record*>(b + L.o_records), b + L.o_bytes,
            reinterpret_cast<LivePackTotal*>(b + L.o_scratch), max_records, max_bytes, L.blocks};
}

// the three launches of a pack: the totals, the scan, the packer's write kernel
template <typename Args>
int live_pack_launch(const Args& a, void (*write_kernel)(Args), const char* launch_write, void* hip_stream) {
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid((uint32_t)a.out.blocks), block(kLivePackSpan);
    hipLaunchKernelGGL(live_pack_total_kernel<Args>, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_pack_total_kernel");
    hipLaunchKernelGGL(live_pack_scan_kernel, dim3(1), block, 0, stream,
                       LivePackScanArgs{a.out.header, a.out.scratch, a.out.max_records, a.out.blocks});
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_pack_scan_kernel");
    hipLaunchKernelGGL(write_kernel, grid, block, 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, launch_write);
    return AFSK_OK;
}

// ---- the write kernels ----

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

__global__ __launch_bounds__(kLivePackSpan) void live_events_write_kernel(LiveEventsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t cc = (int64_t)blockIdx.x * kLivePackSpan + threadIdx.x;
    const int c = cc < a.n ? (int)cc : a.n;
    int32_t e, te;
    int64_t kb, tb;
    live_events_channel(a, c, e, kb);
    int32_t ie = e;
    int64_t ib = kb;
    live_pack_block_scan(ie, ib, te, tb);
    if (te == 0) return;                                // (uniform over the block)
    const LivePackTotal before = a.out.scratch[blockIdx.x];
    const int64_t first = before.records + ie - e;      // the index of this channel's first record
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
            const bool fits = off + kept <= a.out.max_bytes;
            if (idx < a.out.max_records) {
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
                    a.out.records[idx] = r;
                    if (!fits && off <= a.out.max_bytes) a.out.header->stored_bytes = off;  // the first payload left out
                }
                if (fits && kept > 0)
                    live_events_copy(a.out.bytes + off, a.out_bytes + (row + k) * a.out_stride, kept, lane);
            } else if (idx == a.out.max_records && off <= a.out.max_bytes && lane == 0) {
                a.out.header->stored_bytes = off;                                        // the first record left out
            }
            off += kept;
        }
    }
}

// every thread writes its own channel's records (two 16-byte stores each) and copies its own few bytes
__global__ __launch_bounds__(kLivePackSpan) void live_segments_write_kernel(LiveSegmentsArgs a) {
    const int64_t cc = (int64_t)blockIdx.x * kLivePackSpan + threadIdx.x;
    const int c = cc < a.n ? (int)cc : a.n;
    int32_t nc, tn, at, e, te;
    int64_t kb, tb;
    bool open;
    live_segments_channel(a, c, nc, tn, at, open, e, kb);
    int32_t ie = e;
    int64_t ib = kb;
    live_pack_block_scan(ie, ib, te, tb);
    if (te == 0) return;                                // (uniform over the block)
    const LivePackTotal before = a.out.scratch[blockIdx.x];
    int64_t idx = before.records + ie - e;              // the index of this channel's first record
    int64_t off = before.bytes + ib - kb;               // and where its bytes start
    const int64_t row = (int64_t)c * a.slots;
    const uint8_t* src = a.tap_bytes + (int64_t)c * a.tap_cap;
    int32_t done = 0;                                   // tap bytes of the records before this one
    for (int k = 0; k < e; k++, idx++) {
        const bool fin = k < nc;
        const int32_t ln = fin ? min(max(a.tap_len[row + k], 0), tn - done) : tn - done;
        if (idx < a.out.max_records) {
            ev_vec16 lo, hi;
            lo.x = (uint32_t)c;
            lo.y = (uint32_t)(fin ? k : -1);
            const int64_t start = fin ? a.burst_start[row + k] : a.open_start[c];
            lo.z = (uint32_t)(uint64_t)start;
            lo.w = (uint32_t)((uint64_t)start >> 32);
            hi.x = fin ? (uint32_t)a.burst_len[row + k] : 0u;
            hi.y = fin ? (uint32_t)a.flags[row + k] : 0u;
            hi.z = (uint32_t)(fin ? a.nbytes[row + k] : a.open_nbytes[c]) - (uint32_t)ln;
            hi.w = (uint32_t)ln;
            ev_vec16* rec = reinterpret_cast<ev_vec16*>(a.out.records + idx);
            rec[0] = lo;
            rec[1] = hi;
            if (off + ln <= a.out.max_bytes) {
                for (int32_t i = 0; i < ln; i++) a.out.bytes[off + i] = src[done + i];
            } else if (off <= a.out.max_bytes) {
                a.out.header->stored_bytes = off;       // the first record whose bytes are left out
            }
        } else if (idx == a.out.max_records && off <= a.out.max_bytes) {
            a.out.header->stored_bytes = off;           // the first record left out
        }
        done += ln;
        off += ln;
    }
}

}  // namespace afsk

extern "C" {

int afsk_live_events_layout(int32_t n_channels, int32_t slots, int32_t max_events, int64_t max_bytes,
                            int64_t* out_records_offset, int64_t* out_payload_offset, int64_t* out_total_bytes) {
    return afsk::live_pack_layout_entry(n_channels, slots, sizeof(afsk_live_event), max_events, max_bytes,
                                        out_records_offset, out_payload_offset, out_total_bytes);
}

int afsk_live_segments_layout(int32_t n_channels, int32_t slots, int32_t max_segments, int64_t max_bytes,
                              int64_t* out_records_offset, int64_t* out_data_offset, int64_t* out_total_bytes) {
    return afsk::live_pack_layout_entry(n_channels, slots, sizeof(afsk_live_segment), max_segments, max_bytes,
                                        out_records_offset, out_data_offset, out_total_bytes);
}

int afsk_live_pack(int32_t n_channels, int32_t slots, const int32_t* n_closed, const int64_t* burst_start,
                   const int32_t* burst_len, const int32_t* flags, const uint8_t* out_bytes, int32_t out_stride,
                   const int32_t* nbytes, const int32_t* nbits, const int32_t* clock_idx, const int32_t* term_frame,
                   const int32_t* status, void* events, int32_t max_events, int64_t max_bytes, void* hip_stream) {
    using namespace afsk;
    LivePackLayout L;
    if (int rc = live_pack_layout(n_channels, slots, sizeof(afsk_live_event), max_events, max_bytes, L)) return rc;
    if (out_stride < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (!n_closed || !burst_start || !burst_len || !flags || (!out_bytes && out_stride != 0) || !nbytes || !nbits ||
        !clock_idx || !term_frame || !status || !events)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if ((uintptr_t)events & 15) return fail(AFSK_E_INVALID_ARG, "the events buffer must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    const LiveEventsArgs a{n_channels, slots, n_closed, burst_start, burst_len, flags, out_bytes, out_stride,
                           nbytes, nbits, clock_idx, term_frame, status,
                           live_pack_out<afsk_live_event>(events, L, max_events, max_bytes)};
    return live_pack_launch(a, live_events_write_kernel, "launch live_events_write_kernel", hip_stream);
}

int afsk_live_pack_tap(int32_t n_channels, int32_t slots, int32_t tap_cap, const int32_t* n_closed,
                       const int64_t* burst_start, const int32_t* burst_len, const int32_t* flags, const int32_t* nbytes,
                       const uint8_t* tap_bytes, const int32_t* tap_n, const int32_t* tap_len, const int64_t* open_start,
                       const int32_t* open_nbytes, void* segments, int32_t max_segments, int64_t max_bytes,
                       void* hip_stream) {
    using namespace afsk;
    LivePackLayout L;
    if (int rc = live_pack_layout(n_channels, slots, sizeof(afsk_live_segment), max_segments, max_bytes, L)) return rc;
    if (tap_cap < 1) return fail(AFSK_E_INVALID_ARG, "tap_cap must be at least 1");
    if (!n_closed || !burst_start || !burst_len || !flags || !nbytes || !tap_bytes || !tap_n || !tap_len ||
        !open_start || !open_nbytes || !segments)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if ((uintptr_t)segments & 15) return fail(AFSK_E_INVALID_ARG, "the segments buffer must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    const LiveSegmentsArgs a{n_channels, slots, tap_cap, n_closed, burst_start, burst_len, flags, nbytes, tap_bytes,
                             tap_n, tap_len, open_start, open_nbytes,
                             live_pack_out<afsk_live_segment>(segments, L, max_segments, max_bytes)};
    return live_pack_launch(a, live_segments_write_kernel, "launch live_segments_write_kernel", hip_stream);
}

}  // extern "C"
