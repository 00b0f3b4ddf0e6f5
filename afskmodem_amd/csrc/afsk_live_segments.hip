// afsk_live_segments.hip -- the packed segment list of a progressive push (afsk_live_segments_layout /
// afsk_live_pack_tap, include/afsk_amd.h): what the payload tap handed out in one push -- per channel the shares of the
// bursts it reported and the share of the burst still recording -- turned into a count, that many fixed-size records and
// the tap bytes back to back, so that the host copies in proportion to what decoded, not to n_channels * tap_cap.
//
// The segments buffer (one caller-provided allocation, 16-byte aligned):
//   [0, 32)                        LiveEventsHeader (the events buffer's header: count, stored, n_bytes, stored_bytes)
//   [32, 32 + 32 * max_segments)   afsk_live_segment records: channel ascending, the slots ascending, the open segment
//   [data_offset, + max_bytes)     the records' bytes back to back in record order
//   [scratch_offset, total)        one LiveEventsTotal (16 bytes) per span of kLiveEventsSpan channels
//
// The per-channel rule (live_segments_channel): nc = clamp(n_closed[c], 0, slots), tn = clamp(tap_n[c], 0, tap_cap);
// slot k < nc takes ln_k = clamp(tap_len[c, k], 0, tn - at) bytes of the tap row from at on, at += ln_k; rest = tn - at
// is the open segment's when rest > 0 and open_start[c] >= 0.  nc final records (length 0 where a burst closed without
// new bytes), then the open one; their bytes are ONE run of the tap row and land as one run of the data part.
//
// Three ordinary launches in order on the caller's stream, a thread per channel, kLiveEventsSpan channels per block
// (the scan helpers are afsk_live_events.hip's):
//   live_segments_total_kernel  block b sums the records and bytes of its span into scratch[b]
//   live_segments_scan_kernel   ONE block replaces every scratch entry by the sums of the entries before it and writes
//                               the header
//   live_segments_write_kernel  block b scans its span, starts at scratch[b]; every thread writes its own channel's
//                               records (two 16-byte stores each) and copies its own few bytes
// No block ever waits for another.  A list of segments is dense whenever the channels are busy -- an open gate gives a
// segment in every push -- so the write is a thread per channel: 64 channels of a wave are written side by side,
// where a wave per channel would take them in 64 rounds of about 14 bytes.
//
// stored_bytes follows the events buffer: record r's bytes start at off_r and are written when r < max_segments and
// off_r + length_r <= max_bytes; the written ones are the first W records and stored_bytes = off_W.  The scan kernel
// writes stored_bytes = n_bytes; when W < count the one thread that holds record W -- record max_segments with
// off <= max_bytes, or an earlier one with off <= max_bytes < off + length -- overwrites it.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end).

namespace afsk {

static_assert(sizeof(afsk_live_segment) == 32 && offsetof(afsk_live_segment, burst_start) == 8 &&
                  offsetof(afsk_live_segment, burst_len) == 16 && offsetof(afsk_live_segment, length) == 28,
              "afsk_live_segment is 32 bytes without padding");

struct LiveSegmentsLayout {
    int64_t o_records, o_data, o_scratch, total, blocks;
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
    LiveEventsHeader* header;
    afsk_live_segment* records;
    uint8_t* data;
    LiveEventsTotal* scratch;
    int32_t max_segments;
    int64_t max_bytes;
    int64_t blocks;
};

// channel c's slots in use, its tap bytes, those of them its final segments take, and whether the rest is an open
// segment; (records, bytes) in e / kb.  Reads n_closed and tap_n, tap_len for k < nc, open_start where rest > 0.
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

__global__ __launch_bounds__(kLiveEventsSpan) void live_segments_total_kernel(LiveSegmentsArgs a) {
    const int64_t c = (int64_t)blockIdx.x * kLiveEventsSpan + threadIdx.x;
    int32_t nc, tn, at, e, te;
    int64_t kb, tb;
    bool open;
    live_segments_channel(a, c < a.n ? (int)c : a.n, nc, tn, at, open, e, kb);
    live_events_block_scan(e, kb, te, tb);
    if (threadIdx.x == 0) a.scratch[blockIdx.x] = LiveEventsTotal{te, tb};
}

__global__ __launch_bounds__(kLiveEventsSpan) void live_segments_scan_kernel(LiveSegmentsArgs a) {
    int64_t carry_e = 0, carry_b = 0;
    for (int64_t base = 0; base < a.blocks; base += kLiveEventsSpan) {
        const int64_t i = base + threadIdx.x;
        LiveEventsTotal t{0, 0};
        if (i < a.blocks) t = a.scratch[i];
        int32_t e = (int32_t)t.events, te;              // (a span holds at most 256 * (slots + 1) < 2^31 records)
        int64_t kb = t.bytes, tb;
        live_events_block_scan(e, kb, te, tb);
        if (i < a.blocks) a.scratch[i] = LiveEventsTotal{carry_e + e - t.events, carry_b + kb - t.bytes};
        carry_e += te;
        carry_b += tb;
    }
    if (threadIdx.x == 0) {
        LiveEventsHeader h;
        h.count = (int32_t)(carry_e < 0x7fffffffll ? carry_e : 0x7fffffffll);    // (saturates: see the header)
        h.stored = (int32_t)(carry_e < a.max_segments ? carry_e : a.max_segments);
        h.n_bytes = carry_b;
        h.stored_bytes = carry_b;                       // (the write kernel corrects it when bytes are left out)
        h.reserved = 0;
        *a.header = h;
    }
}

__global__ __launch_bounds__(kLiveEventsSpan) void live_segments_write_kernel(LiveSegmentsArgs a) {
    const int64_t cc = (int64_t)blockIdx.x * kLiveEventsSpan + threadIdx.x;
    const int c = cc < a.n ? (int)cc : a.n;
    int32_t nc, tn, at, e, te;
    int64_t kb, tb;
    bool open;
    live_segments_channel(a, c, nc, tn, at, open, e, kb);
    int32_t ie = e;
    int64_t ib = kb;
    live_events_block_scan(ie, ib, te, tb);
    if (te == 0) return;                                // (uniform over the block)
    const LiveEventsTotal before = a.scratch[blockIdx.x];
    int64_t idx = before.events + ie - e;               // the index of this channel's first record
    int64_t off = before.bytes + ib - kb;               // and where its bytes start
    const int64_t row = (int64_t)c * a.slots;
    const uint8_t* src = a.tap_bytes + (int64_t)c * a.tap_cap;
    int32_t done = 0;                                   // tap bytes of the records before this one
    for (int k = 0; k < e; k++, idx++) {
        const bool fin = k < nc;
        const int32_t ln = fin ? min(max(a.tap_len[row + k], 0), tn - done) : tn - done;
        if (idx < a.max_segments) {
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
            ev_vec16* rec = reinterpret_cast<ev_vec16*>(a.records + idx);
            rec[0] = lo;
            rec[1] = hi;
            if (off + ln <= a.max_bytes) {
                for (int32_t i = 0; i < ln; i++) a.data[off + i] = src[done + i];
            } else if (off <= a.max_bytes) {
                a.header->stored_bytes = off;           // the first record whose bytes are left out
            }
        } else if (idx == a.max_segments && off <= a.max_bytes) {
            a.header->stored_bytes = off;               // the first record left out
        }
        done += ln;
        off += ln;
    }
}

// AFSK_E_INVALID_ARG unless the sizes are those afsk_live_segments_layout accepts (afsk_live_events_layout's rules);
// the layout in L
inline int live_segments_layout(int32_t n_channels, int32_t slots, int32_t max_segments, int64_t max_bytes,
                                LiveSegmentsLayout& L) {
    LiveEventsLayout E;
    if (int rc = live_events_layout(n_channels, slots, max_segments, max_bytes, E)) return rc;
    L.blocks = E.blocks;
    L.o_records = (int64_t)sizeof(LiveEventsHeader);
    L.o_data = L.o_records + (int64_t)sizeof(afsk_live_segment) * max_segments;
    L.o_scratch = (L.o_data + max_bytes + 15) & ~15ll;
    L.total = L.o_scratch + (int64_t)sizeof(LiveEventsTotal) * L.blocks;
    return AFSK_OK;
}

}  // namespace afsk

extern "C" {

int afsk_live_segments_layout(int32_t n_channels, int32_t slots, int32_t max_segments, int64_t max_bytes,
                              int64_t* out_records_offset, int64_t* out_data_offset, int64_t* out_total_bytes) {
    afsk::LiveSegmentsLayout L;
    if (int rc = afsk::live_segments_layout(n_channels, slots, max_segments, max_bytes, L)) return rc;
    if (!out_records_offset || !out_data_offset || !out_total_bytes)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out_records_offset = L.o_records;
    *out_data_offset = L.o_data;
    *out_total_bytes = L.total;
    return AFSK_OK;
}

int afsk_live_pack_tap(int32_t n_channels, int32_t slots, int32_t tap_cap, const int32_t* n_closed,
                       const int64_t* burst_start, const int32_t* burst_len, const int32_t* flags, const int32_t* nbytes,
                       const uint8_t* tap_bytes, const int32_t* tap_n, const int32_t* tap_len, const int64_t* open_start,
                       const int32_t* open_nbytes, void* segments, int32_t max_segments, int64_t max_bytes,
                       void* hip_stream) {
    using namespace afsk;
    LiveSegmentsLayout L;
    if (int rc = live_segments_layout(n_channels, slots, max_segments, max_bytes, L)) return rc;
    if (tap_cap < 1) return fail(AFSK_E_INVALID_ARG, "tap_cap must be at least 1");
    if (!n_closed || !burst_start || !burst_len || !flags || !nbytes || !tap_bytes || !tap_n || !tap_len ||
        !open_start || !open_nbytes || !segments)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if ((uintptr_t)segments & 15) return fail(AFSK_E_INVALID_ARG, "the segments buffer must be 16-byte aligned");
    if (int rc = require_device()) return rc;
    uint8_t* sg = static_cast<uint8_t*>(segments);
    const LiveSegmentsArgs a{n_channels, slots, tap_cap, n_closed, burst_start, burst_len, flags, nbytes, tap_bytes,
                             tap_n, tap_len, open_start, open_nbytes, reinterpret_cast<LiveEventsHeader*>(sg),
                             reinterpret_cast<afsk_live_segment*>(sg + L.o_records), sg + L.o_data,
                             reinterpret_cast<LiveEventsTotal*>(sg + L.o_scratch), max_segments, max_bytes, L.blocks};
    hipStream_t stream = (hipStream_t)hip_stream;
    const dim3 grid((uint32_t)L.blocks), block(kLiveEventsSpan);
    hipLaunchKernelGGL(live_segments_total_kernel, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_segments_total_kernel");
    hipLaunchKernelGGL(live_segments_scan_kernel, dim3(1), block, 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_segments_scan_kernel");
    hipLaunchKernelGGL(live_segments_write_kernel, grid, block, 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "launch live_segments_write_kernel");
    return AFSK_OK;
}

}  // extern "C"
