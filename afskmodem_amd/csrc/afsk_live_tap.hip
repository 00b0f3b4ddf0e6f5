// afsk_live_tap.hip -- the streaming live receiver's payload tap (afsk_live_tap_layout / afsk_live_create_stream_tap /
// afsk_live_push_tap, include/afsk_amd.h): every push also hands out, per channel, the payload bytes the demodulator
// committed during that push, so a byte decoded in the first second of a long burst reaches the caller with the push
// that decoded it, and a payload of any length is received whatever max_payload_len is.
//
// A tapped receiver is a streaming receiver (afsk_live_stream.hip) with the same state (afsk_live_stream_layout) and
// the same kernels' walk and sink; its tapped push launches the sink's tapped instantiation, LiveStreamSinkT<true>,
// which differs from the untapped one in four places:
//   step     a committed byte (hi << 4 | nib, also one at or past max_payload_len) is appended to the channel's tap row
//   report   tap_len of the slot = the bytes appended since the previous report of this push (a burst longer than
//            AFSK_MAX_STREAM_LEN reports 0: what this push appended for it is withdrawn)
//   finish   tap_n, and the open burst's start and byte count
//   clear    tap_len 0 for the unused slots
// so a row reads [slot 0][slot 1] ... [open burst], the slots' shares given by tap_len.  An untapped push
// (afsk_live_push) of a tapped receiver is the streaming receiver's push: the bytes it commits are not handed out.
//
// The row's capacity: a push walks at most K = (2047 + max_chunk_len) / 2048 blocks, and the symbols it commits end
// inside those blocks or, while block 0 of a burst waits for the clock search, the one block before them: the bursts
// of one push commit at most (K + 1) * 2048 / bf symbols in all (a burst that continues commits at most
// blocks * 2048 / bf + 1 <= (blocks + 1) * 2048 / bf, a burst that opens at most blocks * 2048 / bf, and bf <= 2000).
// A byte takes 14 data symbols; only the first burst of a push can complete a byte begun in an earlier push.  So
//   tap_cap = ((K + 1) * 2048 / bf_min) / 14 + 1          (AFSK_LIVE_TAP_CAP, bf_min: the receiver's smallest bit_frames)
// and the sink checks the row's end before every store all the same.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), after
// afsk_live_stream.hip.

namespace afsk {

__global__ __launch_bounds__(256) void live_stream_tap_kernel(LiveStreamArgs a, LiveTapArgs t) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSinkT<true> sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    sk.tp.T = t;
    live_gate_walk(a.g, sk);
}

// the tapped receiver with a threshold pair per channel
__global__ __launch_bounds__(256) void live_stream_tap_thr_kernel(LiveStreamArgs a, LiveTapArgs t,
                                                                  const int32_t* thr_start, const int32_t* thr_end) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSinkT<true> sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    sk.tp.T = t;
    live_gate_walk<true>(a.g, sk, thr_start, thr_end);
}

// AFSK_LIVE_TAP_CAP after afsk_live_stream_layout's checks
inline int live_tap_cap(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len, int32_t min_bit_frames,
                        int32_t& cap) {
    LiveStreamLayout L;
    if (int rc = live_stream_layout(n_channels, max_payload_len, max_chunk_len, L)) return rc;
    if (!bf_valid(min_bit_frames)) return fail_bit_frames();
    cap = AFSK_LIVE_TAP_CAP(max_chunk_len, min_bit_frames);
    return AFSK_OK;
}

}  // namespace afsk

extern "C" {

int afsk_live_tap_layout(int32_t n_channels, int32_t max_payload_len, int32_t max_chunk_len, int32_t min_bit_frames,
                         int32_t* out_tap_cap) {
    int32_t cap = 0;
    if (int rc = afsk::live_tap_cap(n_channels, max_payload_len, max_chunk_len, min_bit_frames, cap)) return rc;
    if (out_tap_cap) *out_tap_cap = cap;
    return AFSK_OK;
}

int afsk_live_create_stream_tap(int32_t n_channels, const int32_t* bit_frames_host, const int32_t* amp_start_host,
                                const int32_t* amp_end_host, int32_t max_payload_len, int32_t max_chunk_len,
                                afsk_live** out) {
    bool same;
    if (int rc = live_check_rates(n_channels, bit_frames_host, out, same)) return rc;
    if (!amp_start_host || !amp_end_host) return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    int32_t cap = 0;
    if (int rc = afsk::live_tap_cap(n_channels, max_payload_len, max_chunk_len,
                                    *std::min_element(bit_frames_host, bit_frames_host + n_channels), cap))
        return rc;
    // the state, rates and thresholds of afsk_live_create_stream_thresholds
    const bool per_channel = !all_equal(amp_start_host, n_channels) || !all_equal(amp_end_host, n_channels);
    if (int rc = live_create({"afsk_live_create_stream_tap", n_channels, bit_frames_host, true, amp_start_host,
                              amp_end_host, per_channel, true, 0, max_payload_len, max_chunk_len}, out))
        return rc;
    (*out)->tap_cap = cap;
    return AFSK_OK;
}

int afsk_live_push_tap(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len, int32_t flush,
                       int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                       uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                       int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                       int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes, int32_t* tap_n, int32_t* tap_len,
                       int64_t* open_start, int32_t* open_nbytes, void* hip_stream) {
    const afsk::DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                               out_corrected, out_margins, margin_stride};
    if (!live) return afsk::fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (live->tap_cap <= 0)
        return afsk::fail(AFSK_E_INVALID_ARG, "afsk_live_push_tap needs a receiver of afsk_live_create_stream_tap");
    if (chunk_len < 0 || chunk_row_stride < 0 || o.negative()) return afsk::fail(AFSK_E_INVALID_ARG, "negative size");
    if (chunk_len > live->max_chunk_len)
        return afsk::fail(AFSK_E_INVALID_ARG, "chunk_len exceeds the receiver's max_chunk_len");
    if ((chunk_len > 0 && !chunk) || !out_n_closed || !out_burst_start || !out_burst_len || !out_flags || o.missing() ||
        !tap_bytes || !tap_n || !tap_len || !open_start || !open_nbytes)
        return afsk::fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (out_margins)
        return afsk::fail(AFSK_E_INVALID_ARG, "a streaming live receiver has no margins: out_margins must be NULL");
    if (int rc = live->state.check_current()) return rc;
    afsk::LiveStreamArgs a;
    if (int rc = afsk::live_stream_args(live, chunk, chunk_row_stride, chunk_len, flush, out_n_closed, out_burst_start,
                                        out_burst_len, out_flags, o, a))
        return rc;
    const afsk::LiveTapArgs t{tap_bytes, live->tap_cap, tap_n, tap_len, open_start, open_nbytes};
    const uint32_t grid = (uint32_t)((live->L.n + 3) / 4);
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (live->per_channel)
        hipLaunchKernelGGL(afsk::live_stream_tap_thr_kernel, dim3(grid), dim3(256), 0, stream, a, t, live->thr_start(),
                           live->thr_end());
    else
        hipLaunchKernelGGL(afsk::live_stream_tap_kernel, dim3(grid), dim3(256), 0, stream, a, t);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? AFSK_OK
                           : afsk::hip_fail(e, live->per_channel ? "launch live_stream_tap_thr_kernel"
                                                                 : "launch live_stream_tap_kernel");
}

}  // extern "C"
