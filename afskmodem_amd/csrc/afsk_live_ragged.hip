// afsk_live_ragged.hip -- the ragged push of the live receivers (afsk_live_push_ragged, include/afsk_amd.h): every
// channel takes its own number of samples from its row of the chunk, and every channel has its own flush bit.
//
// live_gate_walk's RAGGED form (afsk_live.hip) reads, per channel c, len_c = clamp(chunk_lens[c], 0, chunk_len) and
// flush_c = flush | flush_mask[c] from DEVICE arrays -- one wave walks one channel, so both are wave-uniform scalar
// loads before the block loop -- and walks with them where the plain form walks with LiveArgs::chunk_len and
// LiveArgs::flush.  Nothing else differs: the sinks never see either value, the state per channel is the plain push's,
// and plain and ragged pushes of one receiver may alternate.
//
// No sample at or beyond column len_c of a row is read: the push walks nblk = (cl + len_c) / 2048 whole blocks (cl:
// carried samples), block b >= 1 is columns [b * 2048 - cl, + 2048) and ends at nblk * 2048 - cl <= len_c, block 0 of
// a push with a carry takes its columns [0, 2048 - cl) sample by sample (2048 - cl <= len_c as nblk >= 1), and the
// carry copy takes columns [nblk * 2048 - cl, len_c).  A channel with len_c = 0 and no flush walks no block, copies
// nothing, and stores the state it loaded (the stored sink's open burst moved to its row's front; the streaming
// sink's window image written back as it was read).
//
// The kernels are the ragged twins of the six gate kernels: stored, streaming and tapped, each with the receiver's one
// threshold pair or a pair per channel.  The stored push's second launch (the demodulator over the slots) is the plain
// push's.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), after
// afsk_live_tap.hip.

namespace afsk {

__global__ __launch_bounds__(256) void live_gate_ragged_kernel(LiveArgs a, const int32_t* chunk_lens,
                                                               const uint8_t* flush_mask) {
    LiveStoreSink sk;
    live_gate_walk<false, true>(a, sk, nullptr, nullptr, chunk_lens, flush_mask);
}

__global__ __launch_bounds__(256) void live_gate_thr_ragged_kernel(LiveArgs a, const int32_t* thr_start,
                                                                   const int32_t* thr_end, const int32_t* chunk_lens,
                                                                   const uint8_t* flush_mask) {
    LiveStoreSink sk;
    live_gate_walk<true, true>(a, sk, thr_start, thr_end, chunk_lens, flush_mask);
}

__global__ __launch_bounds__(256) void live_stream_ragged_kernel(LiveStreamArgs a, const int32_t* chunk_lens,
                                                                 const uint8_t* flush_mask) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSink sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    live_gate_walk<false, true>(a.g, sk, nullptr, nullptr, chunk_lens, flush_mask);
}

__global__ __launch_bounds__(256) void live_stream_thr_ragged_kernel(LiveStreamArgs a, const int32_t* thr_start,
                                                                     const int32_t* thr_end, const int32_t* chunk_lens,
                                                                     const uint8_t* flush_mask) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSink sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    live_gate_walk<true, true>(a.g, sk, thr_start, thr_end, chunk_lens, flush_mask);
}

__global__ __launch_bounds__(256) void live_stream_tap_ragged_kernel(LiveStreamArgs a, LiveTapArgs t,
                                                                     const int32_t* chunk_lens,
                                                                     const uint8_t* flush_mask) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSinkT<true> sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    sk.tp.T = t;
    live_gate_walk<false, true>(a.g, sk, nullptr, nullptr, chunk_lens, flush_mask);
}

__global__ __launch_bounds__(256) void live_stream_tap_thr_ragged_kernel(LiveStreamArgs a, LiveTapArgs t,
                                                                         const int32_t* thr_start,
                                                                         const int32_t* thr_end,
                                                                         const int32_t* chunk_lens,
                                                                         const uint8_t* flush_mask) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * kStreamWinLds];
    LiveStreamSinkT<true> sk{a, reinterpret_cast<int16_t*>(lds + (threadIdx.x >> 6) * kStreamWinLds)};
    sk.tp.T = t;
    live_gate_walk<true, true>(a.g, sk, thr_start, thr_end, chunk_lens, flush_mask);
}

}  // namespace afsk

extern "C" {

int afsk_live_push_ragged(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len,
                          const int32_t* d_chunk_lens_or_null, int32_t flush, const uint8_t* d_flush_mask_or_null,
                          int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                          uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                          int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                          int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes, int32_t* tap_n,
                          int32_t* tap_len, int64_t* open_start, int32_t* open_nbytes, void* hip_stream) {
    const afsk::DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                               out_corrected, out_margins, margin_stride};
    if (!live) return afsk::fail(AFSK_E_INVALID_ARG, "null live receiver");
    if (int rc = afsk::live_push_checks(live, chunk, chunk_row_stride, chunk_len, out_n_closed, out_burst_start,
                                        out_burst_len, out_flags, o))
        return rc;
    const int n_tap = (tap_bytes != nullptr) + (tap_n != nullptr) + (tap_len != nullptr) + (open_start != nullptr) +
                      (open_nbytes != nullptr);
    if (n_tap != 0 && n_tap != 5)
        return afsk::fail(AFSK_E_INVALID_ARG, "the five tap outputs must be all NULL or all given");
    const bool tapped = n_tap == 5;
    if (tapped && live->tap_cap <= 0)
        return afsk::fail(AFSK_E_INVALID_ARG, "tap outputs need a receiver of afsk_live_create_stream_tap");
    if (int rc = live->state.check_current()) return rc;
    const uint32_t grid = (uint32_t)((live->L.n + 3) / 4);
    const hipStream_t st = (hipStream_t)hip_stream;
    const int32_t* lens = d_chunk_lens_or_null;
    const uint8_t* mask = d_flush_mask_or_null;
    if (live->max_payload_len >= 0) {
        afsk::LiveStreamArgs a;
        if (int rc = afsk::live_stream_args(live, chunk, chunk_row_stride, chunk_len, flush, out_n_closed,
                                            out_burst_start, out_burst_len, out_flags, o, a))
            return rc;
        const afsk::LiveTapArgs t{tap_bytes, live->tap_cap, tap_n, tap_len, open_start, open_nbytes};
        const char* what;
        if (tapped && live->per_channel) {
            what = "launch live_stream_tap_thr_ragged_kernel";
            hipLaunchKernelGGL(afsk::live_stream_tap_thr_ragged_kernel, dim3(grid), dim3(256), 0, st, a, t,
                               live->thr_start(), live->thr_end(), lens, mask);
        } else if (tapped) {
            what = "launch live_stream_tap_ragged_kernel";
            hipLaunchKernelGGL(afsk::live_stream_tap_ragged_kernel, dim3(grid), dim3(256), 0, st, a, t, lens, mask);
        } else if (live->per_channel) {
            what = "launch live_stream_thr_ragged_kernel";
            hipLaunchKernelGGL(afsk::live_stream_thr_ragged_kernel, dim3(grid), dim3(256), 0, st, a, live->thr_start(),
                               live->thr_end(), lens, mask);
        } else {
            what = "launch live_stream_ragged_kernel";
            hipLaunchKernelGGL(afsk::live_stream_ragged_kernel, dim3(grid), dim3(256), 0, st, a, lens, mask);
        }
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, what);
    }
    afsk::LiveArgs g;
    afsk::live_stored_args(live, chunk, chunk_row_stride, chunk_len, flush, out_n_closed, out_burst_start,
                           out_burst_len, out_flags, g);
    if (live->per_channel)
        hipLaunchKernelGGL(afsk::live_gate_thr_ragged_kernel, dim3(grid), dim3(256), 0, st, g, live->thr_start(),
                           live->thr_end(), lens, mask);
    else
        hipLaunchKernelGGL(afsk::live_gate_ragged_kernel, dim3(grid), dim3(256), 0, st, g, lens, mask);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return afsk::hip_fail(e, live->per_channel ? "launch live_gate_thr_ragged_kernel"
                                                   : "launch live_gate_ragged_kernel");
    return afsk::live_stored_demod(live, g, o, st);
}

}  // extern "C"
