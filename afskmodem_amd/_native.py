"""ctypes binding of csrc/libafsk_amd.so (C-ABI: include/afsk_amd.h).

There is deliberately no fallback: if the HIP library is missing or no MI355X is
visible, every compute entry raises.  Nothing here (or anywhere in this package)
touches ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AFSK_AMD_LIB: another build of the same library (kernel A/B runs of bench.py with tools/build_variant.sh)
LIB_PATH = os.environ.get("AFSK_AMD_LIB") or os.path.join(_HERE, "csrc", "libafsk_amd.so")

OK = 0
E_INVALID_ARG, E_INVALID_BAUD, E_NO_DEVICE, E_HIP, E_HOST = -1, -2, -3, -4, -5
ST_OK, ST_TOO_SHORT, ST_NO_DATA, ST_INVALID_BAUD, ST_BAD_LENGTH = 0, 1, 2, 3, 4
WAV_OK = 0
WAV_SLOT = 5

SAMPLE_RATE = 48000
SYNC_WINDOW = 4096
MAX_STREAM_LEN = (1 << 30) - (1 << 15)      # AFSK_MAX_STREAM_LEN: 32-bit byte offsets in the kernels


class AfskNativeError(RuntimeError):
    """A C-ABI call returned a negative code."""

    def __init__(self, code: int, message: str):
        super().__init__(f"libafsk_amd error {code}: {message}")
        self.code = code


_lib = None

_i16p = C.POINTER(C.c_int16)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

# name -> (restype, argtypes); mirrors include/afsk_amd.h one to one
SIGNATURES = {
    "afsk_version": (C.c_int, []),
    "afsk_last_error": (C.c_int, [C.c_char_p, C.c_int]),
    "afsk_device_count": (C.c_int, []),
    "afsk_sync": (C.c_int, [C.c_void_p]),
    "afsk_demod_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_demod_batch_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_void_p]),
    "afsk_demod_batch_uniform": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_void_p]),
    "afsk_group_plan_create": (C.c_int, [_i32p, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_group_plan_create_ragged": (C.c_int, [_i32p, _i32p, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_group_plan_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i32p, C.c_int32]),
    "afsk_group_plan_destroy": (C.c_int, [C.c_void_p]),
    "afsk_demod_batch_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p]),
    "afsk_demod_batch_host": (C.c_int, [_i16p, C.c_int64, _i64p, _i32p, _i32p, C.c_int32,
                                        C.c_int32, _u8p, C.c_int32, _i32p, _i32p, _i32p, _i32p,
                                        _i32p]),
    "afsk_demod_streams_host": (C.c_int, [C.POINTER(C.c_void_p), _i32p, _i32p, C.c_int32, C.c_int32,
                                          _u8p, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "afsk_host_scratch_release": (C.c_int, []),
    "afsk_wav_probe": (C.c_int, [C.POINTER(C.c_char_p), C.c_int32, _i64p, _i64p, _i32p]),
    "afsk_file_sizes": (C.c_int, [C.POINTER(C.c_char_p), C.c_int32, _i64p]),
    "afsk_wav_ingest": (C.c_int, [C.POINTER(C.c_char_p), C.c_int32, _i64p, _i64p, C.c_void_p, C.c_int64,
                                  _i64p, _i64p, _i32p]),
    "afsk_wav_egress": (C.c_int, [C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, _i64p, _i32p, _i32p]),
    "afsk_wav_upload": (C.c_int, [C.POINTER(C.c_char_p), _i64p, _i64p, _i64p, C.c_int32, C.c_void_p,
                                  C.c_int64]),
    "afsk_modulate_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p]),
    "afsk_gate_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_gate_batch_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_add_noise_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]),
}


# The sequence-parallel entries (afsk_split_plan_* / afsk_demod_batch_split), bound by lib() like SIGNATURES but kept
# in a table of their own: SIGNATURES is also resolved against builds that do not contain them.
SPLIT_SIGNATURES = {
    "afsk_split_plan_create": (C.c_int, [_i32p, _i32p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_split_plan_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i64p]),
    "afsk_split_plan_destroy": (C.c_int, [C.c_void_p]),
    "afsk_split_scratch_bytes": (C.c_int, [_i32p, _i32p, C.c_int32, C.c_int32, _i64p, _i32p]),
    "afsk_demod_batch_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
}


# The live receiver (afsk_live_*), bound by lib() from a table of its own for the same reason.
LIVE_SIGNATURES = {
    "afsk_live_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i32p, _i64p]),
    "afsk_live_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_void_p)]),
    "afsk_live_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i64p]),
    "afsk_live_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "afsk_live_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_live_destroy": (C.c_int, [C.c_void_p]),
}
LIVE_OPEN_END, LIVE_OVERFLOW = 1, 2          # AFSK_LIVE_* flags


# The live transmitter (afsk_live_tx_*), bound by lib() from a table of its own for the same reason.
LIVE_TX_SIGNATURES = {
    "afsk_live_tx_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i64p]),
    "afsk_live_tx_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_live_tx_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i64p]),
    "afsk_live_tx_submit": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_live_tx_pull": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "afsk_live_tx_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_live_tx_destroy": (C.c_int, [C.c_void_p]),
}
# AFSK_LIVE_TX_* submit statuses
LIVE_TX_QUEUED, LIVE_TX_QUEUE_FULL, LIVE_TX_TOO_LONG, LIVE_TX_BAD_CHANNEL, LIVE_TX_UNSORTED = 0, 1, 2, 3, 4


# The live objects with a rate per channel (afsk_live_create_mixed, afsk_live_tx_create_mixed,
# afsk_live_tx_state_bytes_mixed), bound by lib() from a table of their own for the same reason.
LIVE_MIXED_SIGNATURES = {
    "afsk_live_create_mixed": (C.c_int, [C.c_int32, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_void_p)]),
    "afsk_live_tx_create_mixed": (C.c_int, [C.c_int32, _i32p, _i32p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_live_tx_state_bytes_mixed": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i64p]),
}


# The streaming live receiver (afsk_live_stream_layout, afsk_live_create_stream), bound by lib() from a table of its own
# for the same reason.
LIVE_STREAM_SIGNATURES = {
    "afsk_live_stream_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _i32p, _i64p]),
    "afsk_live_create_stream": (C.c_int, [C.c_int32, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_void_p)]),
}


# The live receivers with a threshold pair per channel (afsk_live_create_thresholds,
# afsk_live_create_stream_thresholds), bound by lib() from a table of their own for the same reason.
LIVE_THRESHOLD_SIGNATURES = {
    "afsk_live_create_thresholds": (C.c_int, [C.c_int32, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_void_p)]),
    "afsk_live_create_stream_thresholds": (C.c_int, [C.c_int32, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                                     C.POINTER(C.c_void_p)]),
}
LIVE_MAX_SQUELCH_CLASSES = 16                # AFSK_LIVE_MAX_SQUELCH_CLASSES

# The host-only view of a stored receiver's squelch classes, likewise.
LIVE_CLASS_SIGNATURES = {
    "afsk_live_squelch_classes": (C.c_int, [C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p]),
}

# The streaming receiver's payload tap (afsk_live_tap_layout, afsk_live_create_stream_tap, afsk_live_push_tap),
# likewise.
LIVE_TAP_SIGNATURES = {
    "afsk_live_tap_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32p]),
    "afsk_live_create_stream_tap": (C.c_int, [C.c_int32, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_void_p)]),
    # afsk_live_push's arguments, the five tap outputs in front of the stream
    "afsk_live_push_tap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The ragged push and pull (afsk_live_push_ragged, afsk_live_tx_pull_ragged: a sample count per channel), likewise.
LIVE_RAGGED_SIGNATURES = {
    # afsk_live_push_tap's arguments, the DEVICE lens behind chunk_len and the DEVICE flush mask behind flush
    "afsk_live_push_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    # afsk_live_tx_pull's arguments, the DEVICE lens behind n_samples
    "afsk_live_tx_pull_ragged": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
}

# The packed event list of a push (afsk_live_events_layout, afsk_live_pack), likewise.
LIVE_EVENT_SIGNATURES = {
    "afsk_live_events_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, _i64p, _i64p]),
    "afsk_live_pack": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int32, C.c_int64, C.c_void_p]),
}

# The packed segment list of a progressive push (afsk_live_segments_layout, afsk_live_pack_tap), likewise.
LIVE_SEGMENT_SIGNATURES = {
    "afsk_live_segments_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, _i64p, _i64p]),
    "afsk_live_pack_tap": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
}

# The rate detector (afsk_detect_rate_batch), likewise.
DETECT_SIGNATURES = {
    "afsk_detect_rate_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _i32p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
DETECT_MAX_CANDIDATES = 36                   # AFSK_DETECT_MAX_CANDIDATES

# The auto-rate streaming live receiver (afsk_live_create_stream_auto, afsk_live_push_auto), likewise.
LIVE_AUTO_SIGNATURES = {
    "afsk_live_create_stream_auto": (C.c_int, [C.c_int32, _i32p, C.c_int32, C.c_int32, _i32p, _i32p, C.c_int32,
                                               C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    # afsk_live_push_ragged's arguments, the two rate outputs in front of the stream
    "afsk_live_push_auto": (C.c_int, LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1][:-1]
                            + [C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The relay submit of the live transmitter (afsk_live_relay_check_map, afsk_live_tx_submit_events), likewise.
LIVE_RELAY_SIGNATURES = {
    "afsk_live_relay_check_map": (C.c_int, [_i32p, C.c_int32, C.c_int32]),
    "afsk_live_tx_submit_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
LIVE_TX_SKIPPED, LIVE_TX_NONE = 5, -1        # AFSK_LIVE_TX_* statuses of afsk_live_tx_submit_events alone

# The rated live transmitter (a rate per queued message: afsk_live_tx_state_bytes_rated, afsk_live_tx_create_rated,
# afsk_live_tx_submit_rated, afsk_live_tx_submit_events_rated), likewise.
LIVE_TX_RATED_SIGNATURES = {
    "afsk_live_tx_state_bytes_rated": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i64p]),
    "afsk_live_tx_create_rated": (C.c_int, [C.c_int32, C.c_int32, _i32p, _i32p, C.c_int32, C.c_int32,
                                            C.POINTER(C.c_void_p)]),
    # afsk_live_tx_submit's arguments, the DEVICE rate_index behind channel
    "afsk_live_tx_submit_rated": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # afsk_live_tx_submit_events' arguments, the DEVICE rate array and its row width behind skip_flags
    "afsk_live_tx_submit_events_rated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]),
}
LIVE_TX_BAD_RATE = 6                         # AFSK_LIVE_TX_BAD_RATE

# Carrier sense (afsk_live_busy, afsk_live_tx_pull_hold), likewise.
LIVE_TX_HOLD_SIGNATURES = {
    "afsk_live_busy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # afsk_live_tx_pull_ragged's arguments, the DEVICE hold and the holdoff behind lens, out_deferred behind out_pending
    "afsk_live_tx_pull_hold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# Half-duplex stations (afsk_live_tx_pull_csma, afsk_live_push_muted, afsk_live_push_auto_muted), likewise.
_ragged_args = LIVE_RAGGED_SIGNATURES["afsk_live_push_ragged"][1]
LIVE_CSMA_SIGNATURES = {
    # afsk_live_tx_pull_hold's arguments, persist, slot and seed behind holdoff, out_on_air behind out_deferred
    "afsk_live_tx_pull_csma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    # afsk_live_push_ragged's / afsk_live_push_auto's arguments, the DEVICE mute ranges behind the flush mask
    "afsk_live_push_muted": (C.c_int, _ragged_args[:7] + [C.c_void_p] + _ragged_args[7:]),
    "afsk_live_push_auto_muted": (C.c_int, _ragged_args[:7] + [C.c_void_p]
                                  + LIVE_AUTO_SIGNATURES["afsk_live_push_auto"][1][7:]),
}

# The live medium (afsk_live_mix, afsk_live_mix_check), likewise.
LIVE_MIX_SIGNATURES = {
    "afsk_live_mix": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_void_p]),
    "afsk_live_mix_check": (C.c_int, [_i32p, _i32p, _i32p, C.c_int32, C.c_int32, C.c_int32]),
}

# The delayed live medium (afsk_live_mix_delayed, afsk_live_mix_delayed_check), likewise: afsk_live_mix's arguments with
# the DEVICE delay array behind the gains and the history and its length behind the position.
LIVE_DELAY_SIGNATURES = {
    "afsk_live_mix_delayed": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p]),
    "afsk_live_mix_delayed_check": (C.c_int, [_i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
}
LIVE_DELAY_MIN_HIST, LIVE_DELAY_MAX_HIST = 8, 1 << 20

# The filtered live medium (afsk_live_mix_filtered, afsk_live_mix_filtered_check), likewise: the delayed entries'
# arguments with the DEVICE filter index per link behind the delays and the filter table (filter_ptr, filter_taps,
# n_filters, n_taps) behind the history's length.
_delayed_args = LIVE_DELAY_SIGNATURES["afsk_live_mix_delayed"][1]
LIVE_FIR_SIGNATURES = {
    "afsk_live_mix_filtered": (C.c_int, _delayed_args[:8] + [C.c_void_p] + _delayed_args[8:19]
                               + [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + _delayed_args[19:]),
    "afsk_live_mix_filtered_check": (C.c_int, [_i32p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, _i32p, _i16p, C.c_int32, C.c_int32]),
}
LIVE_FIR_MAX_TAPS, LIVE_FIR_MAX_L1, LIVE_FIR_UNITY = 256, 65535, 16384

# The faded live medium (afsk_live_mix_faded, afsk_live_mix_faded_check), likewise: the filtered entry's arguments with
# the DEVICE fade tables (link_fade, link_fade_offset, fade_ptr, fade_shift, fade_knots, n_fades, n_knots) behind
# n_taps; the check takes h_link_fade behind h_link_filter and (fade_ptr, fade_shift, n_fades, n_knots) at its end.
_filtered_args = LIVE_FIR_SIGNATURES["afsk_live_mix_filtered"][1]
_filtered_check_args = LIVE_FIR_SIGNATURES["afsk_live_mix_filtered_check"][1]
LIVE_FADE_SIGNATURES = {
    "afsk_live_mix_faded": (C.c_int, _filtered_args[:-1] + [C.c_void_p] * 5 + [C.c_int32, C.c_int32]
                            + _filtered_args[-1:]),
    "afsk_live_mix_faded_check": (C.c_int, _filtered_check_args[:5] + [_i32p] + _filtered_check_args[5:]
                                  + [_i32p, _i32p, C.c_int32, C.c_int32]),
}
LIVE_FADE_MAX_KNOTS, LIVE_FADE_MIN_SHIFT, LIVE_FADE_MAX_SHIFT, LIVE_FADE_MAX_GAIN = 65536, 3, 15, 65535

# The duplicate filter (afsk_live_dedup_*, afsk_live_tx_submit_events_kept), likewise.
LIVE_DEDUP_SIGNATURES = {
    "afsk_live_dedup_layout": (C.c_int, [C.c_int32, C.c_int32, _i64p]),
    "afsk_live_dedup_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_live_dedup_destroy": (C.c_int, [C.c_void_p]),
    "afsk_live_dedup_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_live_dedup_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "afsk_live_dedup_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "afsk_live_dedup_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int64, C.c_void_p, C.c_void_p]),
    "afsk_live_dedup_note": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    # afsk_live_tx_submit_events_rated's arguments, the DEVICE keep array behind rx_slots
    "afsk_live_tx_submit_events_kept": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
LIVE_DEDUP_NONE, LIVE_DEDUP_DUP, LIVE_DEDUP_NEW, LIVE_DEDUP_PASS = -1, 0, 1, 2     # AFSK_LIVE_DEDUP_* verdicts
LIVE_DEDUP_MAX_DEPTH = 64
LIVE_TX_DUPLICATE = 7                        # AFSK_LIVE_TX_DUPLICATE


class LiveLevelParams(C.Structure):
    """afsk_live_level_params: the level tracker's eight parameters, passed by value."""
    _fields_ = [(name, C.c_int32) for name in ("start_q15", "end_q15", "floor_start_q8", "floor_end_q8", "min_start",
                                               "min_end", "decay_shift", "rise_shift")]


# The level tracker (afsk_live_create_stream_leveled, afsk_live_level_check, afsk_live_level, afsk_live_level_reset),
# likewise.
LIVE_LEVEL_SIGNATURES = {
    # afsk_live_create_stream_auto's arguments, the HOST bit_frames (or NULL) behind n_channels
    "afsk_live_create_stream_leveled": (C.c_int, [C.c_int32, _i32p, _i32p, C.c_int32, C.c_int32, _i32p, _i32p,
                                                  C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "afsk_live_level_check": (C.c_int, [LiveLevelParams]),
    "afsk_live_level": (C.c_int, [C.c_void_p, C.c_void_p, LiveLevelParams, C.c_void_p, C.c_int64, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "afsk_live_level_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
}


def lib() -> C.CDLL:
    """Load the HIP shared library, failing loudly when it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with afskmodem_amd/csrc/build.sh "
                "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in (*SIGNATURES.items(), *SPLIT_SIGNATURES.items(), *LIVE_SIGNATURES.items(),
                                  *LIVE_TX_SIGNATURES.items(), *LIVE_MIXED_SIGNATURES.items(),
                                  *LIVE_STREAM_SIGNATURES.items(), *LIVE_THRESHOLD_SIGNATURES.items(),
                                  *LIVE_CLASS_SIGNATURES.items(), *LIVE_TAP_SIGNATURES.items(),
                                  *LIVE_RAGGED_SIGNATURES.items(), *LIVE_EVENT_SIGNATURES.items(),
                                  *LIVE_SEGMENT_SIGNATURES.items(), *DETECT_SIGNATURES.items(),
                                  *LIVE_AUTO_SIGNATURES.items(), *LIVE_RELAY_SIGNATURES.items(),
                                  *LIVE_TX_RATED_SIGNATURES.items(), *LIVE_TX_HOLD_SIGNATURES.items(),
                                  *LIVE_CSMA_SIGNATURES.items(), *LIVE_MIX_SIGNATURES.items(),
                                  *LIVE_DEDUP_SIGNATURES.items(), *LIVE_DELAY_SIGNATURES.items(),
                                  *LIVE_FIR_SIGNATURES.items(), *LIVE_FADE_SIGNATURES.items(),
                                  *LIVE_LEVEL_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    lib().afsk_last_error(buf, len(buf))
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != OK:
        raise AfskNativeError(rc, last_error())


def device_count() -> int:
    return int(lib().afsk_device_count())


def require_device() -> None:
    if device_count() <= 0:
        raise AfskNativeError(E_NO_DEVICE, "no HIP device visible: afskmodem_amd has no CPU fallback")
