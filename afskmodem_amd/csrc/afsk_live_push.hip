// afsk_live_push.hip -- every live receiver's push (afsk_live_push, afsk_live_push_tap, afsk_live_push_ragged,
// afsk_live_push_auto, afsk_live_push_muted, afsk_live_push_auto_muted, include/afsk_amd.h): one kernel template (and its
// muted twin), one table of their instantiations, one host path.
//
// live_push_kernel<Sink, PER_CHANNEL, RAGGED> builds the sink from its argument struct and runs live_gate_walk
// (afsk_live.hip) with it.  The three sinks -- LiveStoreSink (afsk_live.hip), LiveStreamSinkT<false> and
// LiveStreamSinkT<true> (afsk_live_stream.hip; the tapped one: afsk_live_tap.hip) -- times the walk's two flags are the
// twelve cells of kLivePushCells; nothing else calls live_gate_walk.  A further sink or flag is a further index of the
// table, not a further copy of the path: the auto-rate receiver's two sinks, LiveAutoSinkT<false> and LiveAutoSinkT<true>
// (afsk_live_auto.hip), are sink kinds 3 and 4 -- eight more cells, launched by afsk_live_push_auto alone.  The muted
// push (afsk_live_push_muted, afsk_live_push_auto_muted) is form 2 of the table's last index: live_push_mute_kernel<Sink,
// PER_CHANNEL>, the ragged walk with its MUTE flag and the mute array as a third argument -- a kernel of its own name, ten
// more cells, so live_push_kernel's instantiations and their names stay what they were.
//
// afsk::live_push does what the three C entries have in common, once: the argument checks, the receiver's device, the
// kernel arguments, the choice of the cell from the receiver's kind and the call's form, the launch and, for a stored
// receiver, the demodulator over the slots (live_stored_demod).  The entries pack their arguments into a LivePushCall.
// A plain push launches a plain cell and a ragged push a ragged one, whatever the receiver: the ragged form's two scalar
// loads per channel are not paid by callers that have no lengths to pass.
//
// This file is compiled as part of afsk_gate.hip's translation unit (see the #include at its end), after the three
// sinks.

namespace afsk {

// the device arrays only some forms of the walk read; null in the others
struct LivePushPtrs {
    const int32_t* thr_start;       // PER_CHANNEL: int32 [n] each
    const int32_t* thr_end;
    const int32_t* chunk_lens;      // RAGGED: int32 [n] or null
    const uint8_t* flush_mask;      // RAGGED: uint8 [n] or null
};

template <class Sink, bool PER_CHANNEL, bool RAGGED>
__global__ __launch_bounds__(256) void live_push_kernel(typename Sink::Args a, LivePushPtrs x) {
    Sink sk(a);
    live_gate_walk<PER_CHANNEL, RAGGED>(Sink::gate(a), sk, x.thr_start, x.thr_end, x.chunk_lens, x.flush_mask);
}

// the muted push: the ragged walk that takes columns [lo', hi') of channel c's row as 0, mute = DEVICE int32 [n, 2]
template <class Sink, bool PER_CHANNEL>
__global__ __launch_bounds__(256) void live_push_mute_kernel(typename Sink::Args a, LivePushPtrs x, const int32_t* mute) {
    Sink sk(a);
    live_gate_walk<PER_CHANNEL, true, true>(Sink::gate(a), sk, x.thr_start, x.thr_end, x.chunk_lens, x.flush_mask, mute);
}

struct LivePushCell {
    void (*kernel)();               // live_push_kernel<...>, called as void (*)(Sink::Args, LivePushPtrs); a muted cell:
                                    // live_push_mute_kernel<...>, void (*)(Sink::Args, LivePushPtrs, const int32_t*)
    const char* what;               // for hip_fail
};
template <class Sink, bool PER_CHANNEL, bool RAGGED>
LivePushCell live_push_cell(const char* what) {
    return {reinterpret_cast<void (*)()>(&live_push_kernel<Sink, PER_CHANNEL, RAGGED>), what};
}
template <class Sink, bool PER_CHANNEL>
LivePushCell live_push_mute_cell(const char* what) {
    return {reinterpret_cast<void (*)()>(&live_push_mute_kernel<Sink, PER_CHANNEL>), what};
}
#define AFSK_LIVE_PUSH_CELLS(Sink, name)                                                                \
    {{live_push_cell<Sink, false, false>("launch live_push_kernel<" name ">"),                          \
      live_push_cell<Sink, false, true>("launch live_push_kernel<" name ", ragged>"),                   \
      live_push_mute_cell<Sink, false>("launch live_push_mute_kernel<" name ">")},                      \
     {live_push_cell<Sink, true, false>("launch live_push_kernel<" name ", per channel>"),              \
      live_push_cell<Sink, true, true>("launch live_push_kernel<" name ", per channel, ragged>"),       \
      live_push_mute_cell<Sink, true>("launch live_push_mute_kernel<" name ", per channel>")}}
enum LiveSinkKind { kLiveStored, kLiveStream, kLiveTapped, kLiveAuto, kLiveAutoTapped };
enum LivePushForm { kLivePlain, kLiveRagged, kLiveMuted };
// [sink kind][a threshold pair per channel][form: plain, ragged, muted]
static const LivePushCell kLivePushCells[5][2][3] = {AFSK_LIVE_PUSH_CELLS(LiveStoreSink, "stored"),
                                                     AFSK_LIVE_PUSH_CELLS(LiveStreamSinkT<false>, "streaming"),
                                                     AFSK_LIVE_PUSH_CELLS(LiveStreamSinkT<true>, "tapped"),
                                                     AFSK_LIVE_PUSH_CELLS(LiveAutoSinkT<false>, "auto"),
                                                     AFSK_LIVE_PUSH_CELLS(LiveAutoSinkT<true>, "auto, tapped")};
#undef AFSK_LIVE_PUSH_CELLS

// mute: the muted cells' third argument (null: a plain or ragged cell)
template <class Args>
hipError_t live_push_launch(const LivePushCell& cell, int64_t n, hipStream_t stream, const Args& a,
                            const LivePushPtrs& x, const int32_t* mute) {
    if (mute)
        hipLaunchKernelGGL(reinterpret_cast<void (*)(Args, LivePushPtrs, const int32_t*)>(cell.kernel),
                           dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, stream, a, x, mute);
    else
        hipLaunchKernelGGL(reinterpret_cast<void (*)(Args, LivePushPtrs)>(cell.kernel), dim3((uint32_t)((n + 3) / 4)),
                           dim3(256), 0, stream, a, x);
    return hipGetLastError();
}

// The gate's output block of a push, and the tap's.
struct LiveGateOutputs {
    int32_t* n_closed;
    int64_t* burst_start;
    int32_t* burst_len;
    int32_t* flags;
    bool missing() const { return !n_closed || !burst_start || !burst_len || !flags; }
};
struct LiveTapOutputs {
    uint8_t* bytes;
    int32_t* n;
    int32_t* len;
    int64_t* open_start;
    int32_t* open_nbytes;
    int given() const {
        return (bytes != nullptr) + (n != nullptr) + (len != nullptr) + (open_start != nullptr) + (open_nbytes != nullptr);
    }
};

// What a push entry asks for.  `ragged`: the ragged cells, with chunk_lens and flush_mask (device arrays, either may be
// null).  `tap_required`: the entry is the tapped push (else the tap outputs may be all null: an untapped push).
// `auto_rate`: the entry is afsk_live_push_auto, with the two per-slot rate outputs.  `muted`: the entry is
// afsk_live_push_muted or afsk_live_push_auto_muted, a ragged push with d_mute (DEVICE int32 [n, 2], not null).
struct LivePushCall {
    const int16_t* chunk;
    int64_t chunk_row_stride;
    int32_t chunk_len;
    int32_t flush;
    bool ragged;
    const int32_t* chunk_lens;
    const uint8_t* flush_mask;
    LiveGateOutputs gate;
    DemodOutputs o;
    LiveTapOutputs tap;
    bool tap_required;
    hipStream_t stream;
    bool auto_rate = false;
    int32_t* out_bit_frames = nullptr;
    int32_t* out_rate_score = nullptr;
    bool muted = false;
    const int32_t* mute = nullptr;
};

// the gate's arguments every receiver has; o_carry: the carry's place in its state
LiveArgs live_gate_args(const afsk_live* live, const LivePushCall& c, int64_t o_carry) {
    uint8_t* d = live->state.ptr();
    LiveArgs g{};
    g.chan = reinterpret_cast<LiveChan*>(d);
    g.carry = reinterpret_cast<int16_t*>(d + o_carry);
    g.chunk = c.chunk_len > 0 ? c.chunk : g.carry;       // (T = 0: never read)
    g.chunk_stride = c.chunk_len > 0 ? c.chunk_row_stride : 0;
    g.chunk_len = c.chunk_len;
    g.flush = c.flush != 0;
    g.n = (int32_t)live->L.n;
    g.slots = (int32_t)live->L.slots;
    g.amp_start = live->amp_start;
    g.amp_end = live->amp_end;
    g.out_n_closed = c.gate.n_closed;
    g.out_burst_start = c.gate.burst_start;
    g.out_burst_len = c.gate.burst_len;
    g.out_flags = c.gate.flags;
    return g;
}

LiveArgs live_stored_args(const afsk_live* live, const LivePushCall& c) {
    const LiveLayout& L = live->L;
    uint8_t* d = live->state.ptr();
    LiveArgs g = live_gate_args(live, c, L.o_carry);
    g.slot_off = reinterpret_cast<int64_t*>(d + L.o_slot_off);
    g.slot_len = reinterpret_cast<int32_t*>(d + L.o_slot_len);
    g.rows = reinterpret_cast<int16_t*>(d + L.o_rows);
    g.row_len = L.row_len;
    g.cap = L.cap_blocks * kListenBlock;
    return g;
}

LiveStreamArgs live_stream_args(const afsk_live* live, const LivePushCall& c) {
    const LiveStreamLayout& L = live->SL;
    uint8_t* d = live->state.ptr();
    const DemodOutputs& o = c.o;
    LiveStreamArgs a{};
    a.g = live_gate_args(live, c, L.o_carry);
    a.dm = reinterpret_cast<StreamDemod*>(d + L.o_demod);
    a.bit_frames = reinterpret_cast<const int32_t*>(d + L.o_bf);
    a.win = reinterpret_cast<int16_t*>(d + L.o_win);
    a.pay = d + L.o_pay;
    a.max_payload = (int32_t)L.max_payload;
    a.out_bytes = o.bytes;
    a.out_stride = o.stride;
    a.out_nbytes = o.nbytes;
    a.out_nbits = o.nbits;
    a.out_clock_idx = o.clock_idx;
    a.out_term_frame = o.term_frame;
    a.out_status = o.status;
    a.out_corrected = o.corrected;
    return a;
}

int live_push(afsk_live* live, const LivePushCall& c) {
    if (!live) return fail(AFSK_E_INVALID_ARG, "null live receiver");
    const DemodOutputs& o = c.o;
    const int n_tap = c.tap.given();
    if (c.chunk_len < 0 || c.chunk_row_stride < 0 || o.negative()) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (c.chunk_len > live->max_chunk_len)
        return fail(AFSK_E_INVALID_ARG, "chunk_len exceeds the receiver's max_chunk_len");
    if ((c.chunk_len > 0 && !c.chunk) || c.gate.missing() || o.missing() || (c.tap_required && n_tap != 5) ||
        (c.auto_rate && (!c.out_bit_frames || !c.out_rate_score)))
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (c.muted && !c.mute)
        return fail(AFSK_E_INVALID_ARG, c.auto_rate ? "afsk_live_push_auto_muted: null pointer argument (d_mute)"
                                                    : "afsk_live_push_muted: null pointer argument (d_mute)");
    const bool is_auto = live->auto_n_cand > 0;
    if (is_auto && !c.auto_rate)
        return fail(AFSK_E_INVALID_ARG, c.muted ? "afsk_live_push_muted: an auto-rate receiver "
                                                  "(afsk_live_create_stream_auto) is pushed with afsk_live_push_auto_muted"
                                                : "an auto-rate receiver (afsk_live_create_stream_auto) is pushed with "
                                                  "afsk_live_push_auto");
    if (!is_auto && c.auto_rate)
        return fail(AFSK_E_INVALID_ARG, c.muted ? "afsk_live_push_auto_muted needs a receiver of "
                                                  "afsk_live_create_stream_auto: this one is pushed with "
                                                  "afsk_live_push_muted"
                                                : "afsk_live_push_auto needs a receiver of afsk_live_create_stream_auto: "
                                                  "this one is pushed with afsk_live_push, afsk_live_push_tap or "
                                                  "afsk_live_push_ragged");
    const bool streaming = live->max_payload_len >= 0;
    if (streaming && o.margins)
        return fail(AFSK_E_INVALID_ARG, "a streaming live receiver has no margins: out_margins must be NULL");
    if (n_tap != 0 && n_tap != 5)
        return fail(AFSK_E_INVALID_ARG, "the five tap outputs must be all NULL or all given");
    const bool tapped = n_tap == 5;
    if (tapped && live->tap_cap <= 0)
        return fail(AFSK_E_INVALID_ARG, c.tap_required
                                            ? "afsk_live_push_tap needs a receiver of afsk_live_create_stream_tap"
                                            : is_auto ? "tap outputs need a receiver of afsk_live_create_stream_auto "
                                                        "with tap = 1"
                                                      : "tap outputs need a receiver of afsk_live_create_stream_tap");
    if (int rc = live->state.check_current()) return rc;

    const LiveSinkKind kind = is_auto ? (tapped ? kLiveAutoTapped : kLiveAuto)
                                      : tapped ? kLiveTapped : streaming ? kLiveStream : kLiveStored;
    const LivePushCell& cell =
        kLivePushCells[kind][live->per_channel][c.muted ? kLiveMuted : c.ragged ? kLiveRagged : kLivePlain];
    LivePushPtrs x{};
    if (live->per_channel) {
        x.thr_start = live->thr_start();
        x.thr_end = live->thr_end();
    }
    if (c.ragged || c.muted) {
        x.chunk_lens = c.chunk_lens;
        x.flush_mask = c.flush_mask;
    }
    const int64_t n = live->L.n;
    const int32_t* mute = c.muted ? c.mute : nullptr;
    LiveArgs g{};
    hipError_t e;
    if (kind == kLiveStored) {
        g = live_stored_args(live, c);
        e = live_push_launch(cell, n, c.stream, g, x, mute);
    } else {
        const LiveStreamArgs s = live_stream_args(live, c);
        const LiveTapArgs t{c.tap.bytes, live->tap_cap, c.tap.n, c.tap.len, c.tap.open_start, c.tap.open_nbytes};
        if (is_auto) {
            LiveAutoDetect d{c.out_bit_frames, c.out_rate_score, live->auto_max_score, live->auto_n_cand, {}};
            std::copy(live->auto_cand, live->auto_cand + live->auto_n_cand, d.cand);
            e = tapped ? live_push_launch(cell, n, c.stream, LiveAutoArgsT<true>{{s, t}, d}, x, mute)
                       : live_push_launch(cell, n, c.stream, LiveAutoArgsT<false>{s, d}, x, mute);
        } else {
            e = tapped ? live_push_launch(cell, n, c.stream, LiveStreamTapArgs{s, t}, x, mute)
                       : live_push_launch(cell, n, c.stream, s, x, mute);
        }
    }
    if (e != hipSuccess) return hip_fail(e, cell.what);
    return streaming ? AFSK_OK : live_stored_demod(live, g, o, c.stream);
}

}  // namespace afsk

extern "C" {

int afsk_live_push(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len, int32_t flush,
                   int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                   uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                   int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                   int32_t* out_margins, int32_t margin_stride, void* hip_stream) {
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, false, nullptr, nullptr,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {}, false, (hipStream_t)hip_stream});
}

int afsk_live_push_tap(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len, int32_t flush,
                       int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                       uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                       int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                       int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes, int32_t* tap_n, int32_t* tap_len,
                       int64_t* open_start, int32_t* open_nbytes, void* hip_stream) {
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, false, nullptr, nullptr,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {tap_bytes, tap_n, tap_len, open_start, open_nbytes}, true, (hipStream_t)hip_stream});
}

int afsk_live_push_ragged(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len,
                          const int32_t* d_chunk_lens_or_null, int32_t flush, const uint8_t* d_flush_mask_or_null,
                          int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                          uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                          int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                          int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes, int32_t* tap_n,
                          int32_t* tap_len, int64_t* open_start, int32_t* open_nbytes, void* hip_stream) {
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, true, d_chunk_lens_or_null,
                                  d_flush_mask_or_null,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {tap_bytes, tap_n, tap_len, open_start, open_nbytes}, false,
                                  (hipStream_t)hip_stream});
}

int afsk_live_push_auto(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len,
                        const int32_t* d_chunk_lens_or_null, int32_t flush, const uint8_t* d_flush_mask_or_null,
                        int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len, int32_t* out_flags,
                        uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                        int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                        int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes, int32_t* tap_n,
                        int32_t* tap_len, int64_t* open_start, int32_t* open_nbytes, int32_t* out_bit_frames,
                        int32_t* out_rate_score, void* hip_stream) {
    // null lengths and a null mask: the plain cells
    const bool ragged = d_chunk_lens_or_null || d_flush_mask_or_null;
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, ragged, d_chunk_lens_or_null,
                                  d_flush_mask_or_null,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {tap_bytes, tap_n, tap_len, open_start, open_nbytes}, false,
                                  (hipStream_t)hip_stream, true, out_bit_frames, out_rate_score});
}

int afsk_live_push_muted(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len,
                         const int32_t* d_chunk_lens_or_null, int32_t flush, const uint8_t* d_flush_mask_or_null,
                         const int32_t* d_mute, int32_t* out_n_closed, int64_t* out_burst_start, int32_t* out_burst_len,
                         int32_t* out_flags, uint8_t* out_bytes, int32_t out_stride, int32_t* out_nbytes,
                         int32_t* out_nbits, int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status,
                         int32_t* out_corrected, int32_t* out_margins, int32_t margin_stride, uint8_t* tap_bytes,
                         int32_t* tap_n, int32_t* tap_len, int64_t* open_start, int32_t* open_nbytes, void* hip_stream) {
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, true, d_chunk_lens_or_null,
                                  d_flush_mask_or_null,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {tap_bytes, tap_n, tap_len, open_start, open_nbytes}, false,
                                  (hipStream_t)hip_stream, false, nullptr, nullptr, true, d_mute});
}

int afsk_live_push_auto_muted(afsk_live* live, const int16_t* chunk, int64_t chunk_row_stride, int32_t chunk_len,
                              const int32_t* d_chunk_lens_or_null, int32_t flush, const uint8_t* d_flush_mask_or_null,
                              const int32_t* d_mute, int32_t* out_n_closed, int64_t* out_burst_start,
                              int32_t* out_burst_len, int32_t* out_flags, uint8_t* out_bytes, int32_t out_stride,
                              int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx, int32_t* out_term_frame,
                              int32_t* out_status, int32_t* out_corrected, int32_t* out_margins, int32_t margin_stride,
                              uint8_t* tap_bytes, int32_t* tap_n, int32_t* tap_len, int64_t* open_start,
                              int32_t* open_nbytes, int32_t* out_bit_frames, int32_t* out_rate_score, void* hip_stream) {
    return afsk::live_push(live, {chunk, chunk_row_stride, chunk_len, flush, true, d_chunk_lens_or_null,
                                  d_flush_mask_or_null,
                                  {out_n_closed, out_burst_start, out_burst_len, out_flags},
                                  {out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame,
                                   out_status, out_corrected, out_margins, margin_stride},
                                  {tap_bytes, tap_n, tap_len, open_start, open_nbytes}, false,
                                  (hipStream_t)hip_stream, true, out_bit_frames, out_rate_score, true, d_mute});
}

}  // extern "C"
