// afsk_capi_internal.h -- host-side pieces the C-ABI translation units share (afsk_capi.hip, afsk_split.hip,
// afsk_live.hip, afsk_live_tx.hip): the library's last-error slot, the exception barrier of the exported entries, the
// argument checks and output fields every demod entry has in common, and the owner of a handle's device state.  Host
// code only; not part of the installed interface.  What only afsk_capi.hip's host entries need lives in four headers
// that file alone includes: afsk_host_pool.h (NUMA probe, I/O pool, parallel copy), afsk_host_staging.h (scratch cache
// and lease, layout check, two-window loop, window planner, ring session), afsk_host_riff.h (RIFF/WAVE) and
// afsk_host_plan.h (rate-grouped dispatch); tests/helpers/capi_host_driver.cpp drives them under the sanitizers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <exception>
#include <new>
#include <string>

#include "../../include/afsk_amd.h"

namespace afsk {

// store msg in the calling thread's afsk_last_error slot, return code
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
// AFSK_E_NO_DEVICE unless a HIP device is visible
int require_device();
// AFSK_E_INVALID_ARG unless the current device is the one a plan was created on
int plan_on_current_device(int plan_device);

// Entries that allocate on the host (std::vector, std::thread): nothing may be thrown across the C boundary.
template <class F>
int no_throw(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(AFSK_E_HOST, "out of host memory");
    } catch (const std::exception& e) {
        return fail(AFSK_E_HOST, std::string("host-side failure: ") + e.what());
    } catch (...) {
        return fail(AFSK_E_HOST, "host-side failure");
    }
}

// an entry that is nothing but that barrier around its implementation
template <class... P, class... A>
int guarded(int (*impl)(P...), A... args) {
    return no_throw([&] { return impl(args...); });
}

// The host side's bit_frames rule (a multiple of 4 with 2*bf < AFSK_SYNC_WINDOW) and its error.
inline bool bf_valid(int32_t bf) { return bf >= 4 && (bf & 3) == 0 && 2 * bf < AFSK_SYNC_WINDOW; }
inline int fail_bit_frames() {
    return fail(AFSK_E_INVALID_BAUD, "bit_frames must be a multiple of 4 with 2*bf < 4096");
}

// The output block of a demod entry: the five int32 arrays, the byte rows and the optional soft outputs.
struct DemodOutputs {
    uint8_t* bytes;
    int32_t stride;
    int32_t* nbytes;
    int32_t* nbits;
    int32_t* clock_idx;
    int32_t* term_frame;
    int32_t* status;
    int32_t* corrected;
    int32_t* margins;
    int32_t margin_stride;

    bool negative() const { return stride < 0 || margin_stride < 0; }
    bool missing() const {
        return !nbytes || !nbits || !clock_idx || !term_frame || !status || (!bytes && stride > 0);
    }
    // launch arguments (DemodArgs or SplitArgs) with the inputs every entry has and these outputs;
    // the margins only with a positive margin_stride
    template <class Args>
    Args args(const int16_t* samples, const int64_t* stream_offset, const int32_t* stream_len, int32_t amp_end,
              int32_t n_streams) const {
        Args a{};
        a.samples = samples; a.stream_offset = stream_offset; a.stream_len = stream_len;
        a.amp_end = amp_end; a.n_streams = n_streams;
        a.out_bytes = bytes; a.out_stride = stride; a.out_nbytes = nbytes; a.out_nbits = nbits;
        a.out_clock_idx = clock_idx; a.out_term_frame = term_frame; a.out_status = status;
        a.out_corrected = corrected;
        a.out_margins = margin_stride > 0 ? margins : nullptr;
        a.margin_stride = margin_stride;
        return a;
    }
};

// out[i] = 0 for i < n: one small kernel on `stream` (afsk_gate.hip).  A weak reference: a host-only test build of
// afsk_capi.hip alone links stub launchers for the kernels of afsk_kernels.h and may not know this one; the library
// always holds it, and a call without it is an error, never a silent skip.
hipError_t launch_clear_i32(int32_t* out, int64_t n, hipStream_t stream) __attribute__((weak));

// out_corrected[s] is 0 for a stream the demodulator refuses, and the one-wave kernels' refusal branch stores the five
// int32 fields only: zero the n entries on the launch's stream ahead of the launch (capture-safe: one more kernel node
// in front of the demod kernel's).  Nothing for a launch without soft outputs.
inline int clear_corrected(int32_t* corrected, int64_t n, hipStream_t stream) {
    if (!corrected || n <= 0) return AFSK_OK;
    if (&launch_clear_i32 == nullptr) return fail(AFSK_E_HOST, "out_corrected: clear_i32_kernel is not linked into this build");
    hipError_t e = launch_clear_i32(corrected, n, stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch clear_i32_kernel (out_corrected)");
}

// The device state of a handle (a split plan, a live receiver or transmitter): one allocation on the device that was
// current at creation, freed with the handle (whose launches the caller has synchronised).  afsk_capi.hip includes
// this header but calls none of it: its test build runs against a fake runtime without hipMemsetAsync.
struct DeviceState {
    int device = -1;
    void* d = nullptr;
    int64_t bytes = 0;

    DeviceState() = default;
    DeviceState(const DeviceState&) = delete;
    DeviceState& operator=(const DeviceState&) = delete;
    ~DeviceState() {
        if (d) (void)hipFree(d);
    }
    uint8_t* ptr() const { return static_cast<uint8_t*>(d); }

    // Synchronous: require a device and record it, allocate `nbytes` (nothing for 0), zero the first `zero_bytes`,
    // upload `host_bytes` of `host` (when not null) at offset `host_at`.  `entry` names the caller in the errors.
    int create(const char* entry, int64_t nbytes, int64_t zero_bytes, const void* host = nullptr, int64_t host_at = 0,
               int64_t host_bytes = 0) {
        if (int rc = require_device()) return rc;
        const std::string name(entry);
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) return hip_fail(e, (name + " (hipGetDevice)").c_str());
        if (nbytes == 0) return AFSK_OK;
        e = hipMalloc(&d, (size_t)nbytes);
        if (e != hipSuccess) { d = nullptr; return hip_fail(e, (name + " (hipMalloc)").c_str()); }
        bytes = nbytes;
        if (zero_bytes > 0) e = hipMemsetAsync(d, 0, (size_t)zero_bytes, nullptr);
        if (e == hipSuccess && host)
            e = hipMemcpyAsync(ptr() + host_at, host, (size_t)host_bytes, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess)
            return hip_fail(e, (name + (zero_bytes > 0 ? " (initialise the state)" : " (upload)")).c_str());
        return AFSK_OK;
    }
    // AFSK_E_NO_DEVICE without a device, AFSK_E_INVALID_ARG unless the current device is the one of the state
    int check_current() const {
        if (int rc = require_device()) return rc;
        return plan_on_current_device(device);
    }
};

}  // namespace afsk
