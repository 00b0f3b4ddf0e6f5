// afsk_live_tap.hip -- the streaming live receiver's payload tap (afsk_live_tap_layout / afsk_live_create_stream_tap /
// afsk_live_push_tap, include/afsk_amd.h): every push also hands out, per channel, the payload bytes the demodulator
// committed during that push, so a byte decoded in the first second of a long burst reaches the caller with the push
// that decoded it, and a payload of any length is received whatever max_payload_len is.
//
// A tapped receiver is a streaming receiver (afsk_live_stream.hip) with the same state (afsk_live_stream_layout) and
// the same walk and sink; its tapped push (afsk_live_push.hip) launches live_push_kernel's cells of the sink's tapped
// instantiation, LiveStreamSinkT<true>, which differs from the untapped one in four places:
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

}  // extern "C"
