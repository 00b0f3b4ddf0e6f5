// afsk_capi.hip -- extern "C" boundary of libafsk_amd.so (see include/afsk_amd.h).
// Host-side argument checks, error strings and kernel launches; no torch types.  What the host entries are made
// of lives in host-only headers that this file alone includes: afsk_host_pool.h (NUMA, I/O pool, parallel copy),
// afsk_host_staging.h (scratch cache, lease, two-window loop, window planner, ring session), afsk_host_riff.h
// (RIFF/WAVE) and afsk_host_plan.h (rate-grouped dispatch).
#include <hip/hip_runtime.h>

#include <sys/uio.h>

#include <chrono>

#include "../../include/afsk_amd.h"
#include "afsk_capi_internal.h"
#include "afsk_kernels.h"
#include "afsk_host_pool.h"      // (the four bring the standard and POSIX headers their own code and the entries use)
#include "afsk_host_staging.h"
#include "afsk_host_riff.h"
#include "afsk_host_plan.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace afsk {

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(AFSK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(AFSK_E_NO_DEVICE, "no HIP device visible: libafsk_amd has no CPU fallback");
    }
    return AFSK_OK;
}

int plan_on_current_device(int plan_device) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != plan_device)
        return fail(AFSK_E_INVALID_ARG, "the plan was created on another device than the current one");
    return AFSK_OK;
}

}  // namespace afsk

using afsk::bf_valid;
using afsk::DemodOutputs;
using afsk::fail;
using afsk::fail_bit_frames;
using afsk::hip_fail;
using afsk::no_throw;
using afsk::require_device;

namespace {

#define AFSK_HIP(call, what)                             \
    do {                                                 \
        hipError_t e_ = (call);                          \
        if (e_ != hipSuccess) { rc = hip_fail(e_, what); goto done; } \
    } while (0)

// The part of the host-buffer entries that follows their argument checks.  Device scratch: samples | meta = offsets,
// len, bf | the index list and bit_frames of a grouped dispatch | out = 5 x int32 [n], bytes [n, stride].
// upload(lease, d_samples, stream) puts the total_samples samples at the start of it, where dev_offset[] points;
// then one H2D of the meta block, the launch, one D2H of all outputs and the scatter into `o` (host arrays).
// `block`: wait for the shared scratch cache (which owns the staging windows) instead of allocating privately.
template <class Upload>
int run_host_entry(int64_t total_samples, const int64_t* dev_offset, const int32_t* stream_len,
                   const int32_t* bit_frames, int32_t amp_end_threshold, int32_t n_streams,
                   const DemodOutputs& o, bool block, Upload&& upload) {
    if (int rc0 = require_device()) return rc0;

    int rc = AFSK_OK;
    const size_t n = (size_t)n_streams;
    const size_t sample_bytes = (size_t)(total_samples > 0 ? total_samples : 1) * 2;
    const size_t bytes_out = n * (size_t)o.stride;
    const size_t o_meta = (sample_bytes + 255) & ~(size_t)255;
    const size_t meta_bytes = n * 16;
    const size_t o_out = o_meta + meta_bytes + n * 8;      // + the index list and bit_frames of a grouped dispatch
    const size_t out_bytes_total = n * 20 + bytes_out;
    hipStream_t stream = nullptr;
    {
        hipError_t e = g_thread_stream.get(&stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithFlags (host-entry stream)");
    }
    ScratchLease lease;
    std::unique_ptr<GroupPlan> plan;      // mixed rates: the host copy of the index list, alive until the final synchronise
    char* d_all = nullptr;
    // host staging: one H2D for the three index arrays, one D2H for all six outputs
    std::vector<char> h_meta(meta_bytes), h_out(out_bytes_total);
    std::memcpy(h_meta.data(), dev_offset, n * 8);
    std::memcpy(h_meta.data() + n * 8, stream_len, n * 4);
    std::memcpy(h_meta.data() + n * 12, bit_frames, n * 4);
    {
        hipError_t e = lease.acquire(o_out + out_bytes_total, &d_all, block);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (host-entry scratch)");
    }
    if ((rc = upload(lease, d_all, stream)) != AFSK_OK) goto done;
    AFSK_HIP(hipMemcpyAsync(d_all + o_meta, h_meta.data(), meta_bytes, hipMemcpyHostToDevice, stream),
             "H2D stream index");
    {
        int32_t* i32 = (int32_t*)(d_all + o_out);
        const DemodOutputs d_out{(uint8_t*)(d_all + o_out + n * 20), o.stride, i32, i32 + n, i32 + 2 * n, i32 + 3 * n,
                                 i32 + 4 * n, nullptr, nullptr, 0};
        rc = demod_device_auto(bit_frames, stream_len, (const int16_t*)d_all, (const int64_t*)(d_all + o_meta),
                               (const int32_t*)(d_all + o_meta + n * 8), amp_end_threshold, n_streams, d_out, stream,
                               (int32_t*)(d_all + o_meta + n * 16), plan);
        if (rc != AFSK_OK) goto done;
    }
    AFSK_HIP(hipMemcpyAsync(h_out.data(), d_all + o_out, out_bytes_total, hipMemcpyDeviceToHost, stream),
             "D2H results");
    AFSK_HIP(hipStreamSynchronize(stream), "hipStreamSynchronize");
    std::memcpy(o.nbytes, h_out.data(), n * 4);
    std::memcpy(o.nbits, h_out.data() + n * 4, n * 4);
    std::memcpy(o.clock_idx, h_out.data() + n * 8, n * 4);
    std::memcpy(o.term_frame, h_out.data() + n * 12, n * 4);
    std::memcpy(o.status, h_out.data() + n * 16, n * 4);
    if (bytes_out > 0) std::memcpy(o.bytes, h_out.data() + n * 20, bytes_out);
done:
    // nothing may still use the scratch, the staging windows or the host vectors when they are released
    if (rc != AFSK_OK) (void)hipStreamSynchronize(stream);
    return rc;   // the lease returns (or frees) the device scratch
}

}  // namespace

extern "C" {

int afsk_version(void) { return AFSK_ABI_VERSION; }

int afsk_last_error(char* buf, int cap) {
    if (buf && cap > 0) {
        std::strncpy(buf, g_last_error.c_str(), (size_t)cap - 1);
        buf[cap - 1] = '\0';
    }
    return (int)g_last_error.size();
}

int afsk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int afsk_sync(void* hip_stream) {
    if (int rc = require_device()) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "hipStreamSynchronize");
}

int afsk_demod_batch(const int16_t* samples, const int64_t* stream_offset,
                     const int32_t* stream_len, const int32_t* bit_frames,
                     int32_t amp_end_threshold, int32_t n_streams, uint8_t* out_bytes,
                     int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                     int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status,
                     void* hip_stream) {
    return afsk_demod_batch_ex(samples, stream_offset, stream_len, bit_frames, amp_end_threshold,
                               n_streams, out_bytes, out_stride, out_nbytes, out_nbits,
                               out_clock_idx, out_term_frame, out_status, nullptr, nullptr, 0,
                               hip_stream);
}

int afsk_demod_batch_ex(const int16_t* samples, const int64_t* stream_offset,
                        const int32_t* stream_len, const int32_t* bit_frames,
                        int32_t amp_end_threshold, int32_t n_streams, uint8_t* out_bytes,
                        int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                        int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status,
                        int32_t* out_corrected, int32_t* out_margins, int32_t margin_stride,
                        void* hip_stream) {
    const DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                         out_corrected, out_margins, margin_stride};
    if (n_streams < 0 || o.negative()) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || !bit_frames || o.missing())
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    if (int rc = afsk::clear_corrected(o.corrected, n_streams, (hipStream_t)hip_stream)) return rc;
    afsk::DemodArgs a = o.args<afsk::DemodArgs>(samples, stream_offset, stream_len, amp_end_threshold, n_streams);
    a.bit_frames = bit_frames;
    hipError_t e = afsk::launch_demod(a, (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch demod_kernel");
}

int afsk_demod_batch_uniform(const int16_t* samples, const int64_t* stream_offset,
                             const int32_t* stream_len, int32_t bit_frames,
                             int32_t amp_end_threshold, int32_t n_streams, uint8_t* out_bytes,
                             int32_t out_stride, int32_t* out_nbytes, int32_t* out_nbits,
                             int32_t* out_clock_idx, int32_t* out_term_frame, int32_t* out_status,
                             int32_t* out_corrected, int32_t* out_margins, int32_t margin_stride,
                             void* hip_stream) {
    const DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                         out_corrected, out_margins, margin_stride};
    if (n_streams < 0 || o.negative()) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (!bf_valid(bit_frames)) return fail_bit_frames();
    if (n_streams == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || o.missing())
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    if (int rc = afsk::clear_corrected(o.corrected, n_streams, (hipStream_t)hip_stream)) return rc;
    afsk::DemodArgs a = o.args<afsk::DemodArgs>(samples, stream_offset, stream_len, amp_end_threshold, n_streams);
    a.uniform_bit_frames = bit_frames;
    hipError_t e = afsk::launch_demod_uniform(a, (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch demod_uniform_kernel");
}

struct afsk_group_plan { GroupPlan p; };

int afsk_group_plan_create(const int32_t* bit_frames_host, int32_t n_streams, afsk_group_plan** out_plan) {
    return afsk_group_plan_create_ragged(bit_frames_host, nullptr, n_streams, out_plan);
}

int afsk_group_plan_create_ragged(const int32_t* bit_frames_host, const int32_t* stream_len_host, int32_t n_streams,
                                  afsk_group_plan** out_plan) {
    if (!out_plan) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    *out_plan = nullptr;
    if (n_streams < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams > 0 && !bit_frames_host) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    return no_throw([&] {
        std::unique_ptr<afsk_group_plan> pl(new afsk_group_plan());
        pl->p.bucket(bit_frames_host, n_streams, stream_len_host);
        hipError_t e = pl->p.materialise(nullptr, nullptr);
        if (e != hipSuccess) return hip_fail(e, "afsk_group_plan_create (index list)");
        *out_plan = pl.release();
        return AFSK_OK;
    });
}

int afsk_group_plan_info(const afsk_group_plan* plan, int32_t* out_n_streams, int32_t* out_n_groups,
                         int32_t* out_group_bit_frames, int32_t* out_group_count, int32_t cap) {
    if (!plan) return fail(AFSK_E_INVALID_ARG, "null plan");
    if (out_n_streams) *out_n_streams = plan->p.n;
    if (out_n_groups) *out_n_groups = (int32_t)plan->p.groups.size();
    for (int32_t k = 0; k < cap && k < (int32_t)plan->p.groups.size(); k++) {
        if (out_group_bit_frames) out_group_bit_frames[k] = plan->p.groups[(size_t)k].bf;
        if (out_group_count) out_group_count[k] = plan->p.groups[(size_t)k].count;
    }
    return AFSK_OK;
}

int afsk_group_plan_destroy(afsk_group_plan* plan) {
    delete plan;      // the index list; the caller has synchronised its launches
    return AFSK_OK;
}

int afsk_demod_batch_grouped(const afsk_group_plan* plan, const int16_t* samples,
                             const int64_t* stream_offset, const int32_t* stream_len,
                             int32_t amp_end_threshold, uint8_t* out_bytes, int32_t out_stride,
                             int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx,
                             int32_t* out_term_frame, int32_t* out_status, int32_t* out_corrected,
                             int32_t* out_margins, int32_t margin_stride, void* hip_stream) {
    const DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                         out_corrected, out_margins, margin_stride};
    if (!plan) return fail(AFSK_E_INVALID_ARG, "null plan");
    if (o.negative()) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (plan->p.n == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || o.missing())
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    if (int rc = afsk::plan_on_current_device(plan->p.device)) return rc;
    if (int rc = afsk::clear_corrected(o.corrected, plan->p.n, (hipStream_t)hip_stream)) return rc;
    hipError_t e = plan->p.launch(o.args<afsk::DemodArgs>(samples, stream_offset, stream_len, amp_end_threshold,
                                                          plan->p.n), (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch demod_kernel (grouped)");
}

static int demod_batch_host_impl(const int16_t* samples, int64_t total_samples,
                                 const int64_t* stream_offset, const int32_t* stream_len,
                                 const int32_t* bit_frames, int32_t amp_end_threshold,
                                 int32_t n_streams, uint8_t* out_bytes, int32_t out_stride,
                                 int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx,
                                 int32_t* out_term_frame, int32_t* out_status) {
    const DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                         nullptr, nullptr, 0};
    if (n_streams < 0 || o.negative() || total_samples < 0)
        return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0) return AFSK_OK;
    if (!stream_offset || !stream_len || !bit_frames || o.missing() || (!samples && total_samples > 0))
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t s = 0; s < n_streams; s++) {
        if (!bf_valid(bit_frames[s])) return fail_bit_frames();
        if (stream_len[s] < 0 || stream_len[s] > AFSK_MAX_STREAM_LEN || stream_offset[s] < 0 ||
            stream_offset[s] + stream_len[s] > total_samples)
            return fail(AFSK_E_INVALID_ARG, "stream outside the sample buffer (or longer than AFSK_MAX_STREAM_LEN)");
    }
    // the caller's buffer is the device layout already: one copy
    return run_host_entry(total_samples, stream_offset, stream_len, bit_frames, amp_end_threshold, n_streams, o,
                          /*block=*/false, [&](ScratchLease&, char* d_samples, hipStream_t stream) {
        if (total_samples == 0) return AFSK_OK;
        hipError_t e = hipMemcpyAsync(d_samples, samples, (size_t)total_samples * 2, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? AFSK_OK : hip_fail(e, "H2D samples");
    });
}

int afsk_demod_batch_host(const int16_t* samples, int64_t total_samples,
                          const int64_t* stream_offset, const int32_t* stream_len,
                          const int32_t* bit_frames, int32_t amp_end_threshold,
                          int32_t n_streams, uint8_t* out_bytes, int32_t out_stride,
                          int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx,
                          int32_t* out_term_frame, int32_t* out_status) {
    return afsk::guarded(demod_batch_host_impl, samples, total_samples, stream_offset, stream_len, bit_frames, amp_end_threshold,
                         n_streams, out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status);
}

int afsk_host_scratch_release(void) {
    std::lock_guard<std::mutex> lk(g_scratch.mu);
    if (g_scratch.ptr) {
        hipError_t e = hipFree(g_scratch.ptr);
        g_scratch.ptr = nullptr;
        g_scratch.cap = 0;
        if (e != hipSuccess) return hip_fail(e, "hipFree (host-entry scratch)");
    }
    for (int k = 0; k < 2; k++) {
        if (g_scratch.stage[k]) { (void)hipHostFree(g_scratch.stage[k]); g_scratch.stage[k] = nullptr; }
        if (g_scratch.stage_free[k]) { (void)hipEventDestroy(g_scratch.stage_free[k]); g_scratch.stage_free[k] = nullptr; }
        if (g_scratch.ring_extra[k]) { (void)hipHostFree(g_scratch.ring_extra[k]); g_scratch.ring_extra[k] = nullptr; }
    }
    for (hipEvent_t& ev : g_scratch.ring_sent)
        if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    return AFSK_OK;
}

static int demod_streams_host_impl(const int16_t* const* streams, const int32_t* stream_len,
                                   const int32_t* bit_frames, int32_t amp_end_threshold,
                                   int32_t n_streams, uint8_t* out_bytes, int32_t out_stride,
                                   int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx,
                                   int32_t* out_term_frame, int32_t* out_status) {
    const DemodOutputs o{out_bytes, out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status,
                         nullptr, nullptr, 0};
    if (n_streams < 0 || o.negative()) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0) return AFSK_OK;
    if (!streams || !stream_len || !bit_frames || o.missing())
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const size_t n = (size_t)n_streams;
    // device layout: every stream starts on a 16-byte boundary
    std::vector<int64_t> h_off(n);
    int64_t total_samples = 0;
    for (size_t s = 0; s < n; s++) {
        if (!bf_valid(bit_frames[s])) return fail_bit_frames();
        if (stream_len[s] < 0 || stream_len[s] > AFSK_MAX_STREAM_LEN || (stream_len[s] > 0 && !streams[s]))
            return fail(AFSK_E_INVALID_ARG, "bad stream length or null stream pointer");
        h_off[s] = total_samples;
        total_samples += ((int64_t)stream_len[s] + 7) & ~(int64_t)7;
    }
    return run_host_entry(total_samples, h_off.data(), stream_len, bit_frames, amp_end_threshold, n_streams, o,
                          /*block=*/true, [&](ScratchLease& lease, char* d_samples, hipStream_t stream) {
        confine_pool_to_device_node();                    // the packing threads belong on the device's socket
        // windows of the device sample range; pieces of streams are packed into a pinned window
        // by the copy threads while the previous window is on the wire
        size_t s_cur = 0;                                  // first stream that may reach into the window
        std::vector<CopyJob> jobs;
        return two_window_loop(lease, stream, 0, (size_t)total_samples * 2, [&](char* st, size_t w0, size_t w1) {
            jobs.clear();
            size_t moved = 0;
            for (size_t s = s_cur; s < n; s++) {
                const size_t b0 = (size_t)h_off[s] * 2, b1 = b0 + (size_t)stream_len[s] * 2;
                if (b0 >= w1) break;
                if (b1 <= w0) { s_cur = s + 1; continue; }
                const size_t lo = std::max(b0, w0), hi = std::min(b1, w1);
                jobs.push_back({st + (lo - w0), (const char*)streams[s] + (lo - b0), hi - lo});
                moved += hi - lo;
            }
            parallel_copy(jobs, moved);
            hipError_t e = hipMemcpyAsync(d_samples + w0, st, w1 - w0, hipMemcpyHostToDevice, stream);
            return e == hipSuccess ? AFSK_OK : hip_fail(e, "H2D samples");
        });
    });
}

int afsk_demod_streams_host(const int16_t* const* streams, const int32_t* stream_len,
                            const int32_t* bit_frames, int32_t amp_end_threshold,
                            int32_t n_streams, uint8_t* out_bytes, int32_t out_stride,
                            int32_t* out_nbytes, int32_t* out_nbits, int32_t* out_clock_idx,
                            int32_t* out_term_frame, int32_t* out_status) {
    return afsk::guarded(demod_streams_host_impl, streams, stream_len, bit_frames, amp_end_threshold, n_streams, out_bytes,
                         out_stride, out_nbytes, out_nbits, out_clock_idx, out_term_frame, out_status);
}

int afsk_wav_probe(const char* const* paths, int32_t n_files, int64_t* out_data_offset,
                   int64_t* out_data_bytes, int32_t* out_status) {
    if (n_files < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_files == 0) return AFSK_OK;
    if (!paths || !out_data_offset || !out_data_bytes || !out_status)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t i = 0; i < n_files; i++)
        if (!paths[i]) return fail(AFSK_E_INVALID_ARG, "null path");
    return no_throw([&] {
        io_pool().run((size_t)n_files, io_threads(), [&](size_t i) {
            out_status[i] = wav_probe_one(paths[i], &out_data_offset[i], &out_data_bytes[i]);
        });
        return AFSK_OK;
    });
}

static int wav_upload_impl(const char* const* paths, const int64_t* data_offset, const int64_t* data_bytes,
                           const int64_t* stream_offset, int32_t n_files, int16_t* d_samples,
                           int64_t capacity_samples) {
    if (n_files < 0 || capacity_samples < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_files == 0) return AFSK_OK;
    if (!paths || !data_offset || !data_bytes || !stream_offset || !d_samples)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const size_t n = (size_t)n_files;
    LayoutCheck layout{"stream", capacity_samples};
    for (size_t s = 0; s < n; s++)
        if (int rc0 = layout.next(paths[s] && data_offset[s] >= 0 && data_bytes[s] >= 0, stream_offset[s], data_bytes[s] / 2))
            return rc0;
    if (int rc0 = require_device()) return rc0;
    int rc = AFSK_OK;
    hipStream_t stream = nullptr;
    {
        hipError_t e = g_thread_stream.get(&stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithFlags (host-entry stream)");
    }
    ScratchLease lease;                                   // (its lock owns the staging windows)
    if (hipError_t e = lease.lock(); e != hipSuccess) return hip_fail(e, "hipMalloc (host-entry scratch)");
    std::vector<int> fds(n, -1);
    std::atomic<int> io_failed{-1};
    struct Piece { size_t file; int64_t file_off; char* dst; size_t bytes; bool last; };
    constexpr size_t kZeroPiece = ~(size_t)0;             // Piece::file of a zero-filled alignment gap
    constexpr size_t kUploadGapFill = 256;
    {
        // windows over the device byte range the streams cover; a window holds whole or partial
        // streams, each read by one pread straight into pinned memory
        size_t s_cur = 0;
        std::vector<Piece> pieces;
        rc = two_window_loop(lease, stream, (size_t)stream_offset[0] * 2, (size_t)layout.end * 2, [&](char* st, size_t w0, size_t w1) {
            pieces.clear();
            for (size_t s = s_cur; s < n; s++) {
                const size_t b0 = (size_t)stream_offset[s] * 2, b1 = b0 + ((size_t)data_bytes[s] & ~(size_t)1);
                if (b0 >= w1) break;
                // the alignment gap behind the stream (up to kGapFill bytes to the next stream's start) is a
                // piece of its own, filled with zeros -- in whichever window(s) it falls
                size_t g1 = b1;
                if (s + 1 < n) {
                    const size_t nb0 = (size_t)stream_offset[s + 1] * 2;
                    if (nb0 > b1 && nb0 - b1 <= kUploadGapFill) g1 = nb0;
                }
                if (g1 <= w0) { s_cur = s + 1; continue; }
                if (b1 > w0) {
                    const size_t lo = std::max(b0, w0), hi = std::min(b1, w1);
                    if (hi > lo) pieces.push_back({s, data_offset[s] + (int64_t)(lo - b0), st + (lo - w0), hi - lo, hi == b1});
                }
                const size_t zlo = std::max(b1, w0), zhi = std::min(g1, w1);
                if (zhi > zlo) pieces.push_back({kZeroPiece, 0, st + (zlo - w0), zhi - zlo, false});
            }
            io_pool().run(pieces.size(), io_threads(), [&](size_t i) {
                const Piece& p = pieces[i];
                if (p.file == kZeroPiece) { std::memset(p.dst, 0, p.bytes); return; }
                if (fds[p.file] < 0) fds[p.file] = open(paths[p.file], O_RDONLY | O_CLOEXEC);
                if (fds[p.file] < 0 || !pread_all(fds[p.file], p.dst, p.bytes, p.file_off))
                    io_failed.store((int)p.file);
                if (p.last && fds[p.file] >= 0) {           // closed here, in parallel, not in a serial loop at the end
                    close(fds[p.file]);
                    fds[p.file] = -1;
                }
            });
            if (io_failed.load() >= 0) return fail(AFSK_E_HOST, std::string("cannot read ") + paths[io_failed.load()]);
            // Only the stream pieces of the window were filled.  Send it as contiguous RUNS of pieces:
            // an alignment gap of up to kGapFill bytes between two streams is zero-filled and travels with
            // the run (one copy per stream would cost more than the transfer); a larger gap -- room the
            // caller keeps for streams it fills some other way -- ends the run and is never written.
            size_t run0 = 0, run1 = 0;                                  // window-relative byte range of the open run
            bool open = false;
            auto send_run = [&] {
                hipError_t e = hipMemcpyAsync((char*)d_samples + w0 + run0, st + run0, run1 - run0, hipMemcpyHostToDevice, stream);
                return e == hipSuccess ? AFSK_OK : hip_fail(e, "H2D samples");
            };
            for (const Piece& p : pieces) {
                const size_t a0 = (size_t)(p.dst - st), a1 = a0 + p.bytes;
                if (open && a0 == run1) {                               // (gaps to be zeroed are pieces themselves)
                    run1 = a1;
                    continue;
                }
                if (open)
                    if (int rc1 = send_run()) return rc1;
                run0 = a0; run1 = a1; open = true;
            }
            return open ? send_run() : AFSK_OK;
        });
    }
    {
        const hipError_t e = hipStreamSynchronize(stream);   // (also after a failure: nothing may still read the staging windows)
        if (e != hipSuccess && rc == AFSK_OK) rc = hip_fail(e, "hipStreamSynchronize");
    }
    for (int fd : fds)
        if (fd >= 0) close(fd);
    return rc;
}

int afsk_wav_upload(const char* const* paths, const int64_t* data_offset, const int64_t* data_bytes,
                    const int64_t* stream_offset, int32_t n_files, int16_t* d_samples,
                    int64_t capacity_samples) {
    return afsk::guarded(wav_upload_impl, paths, data_offset, data_bytes, stream_offset, n_files, d_samples, capacity_samples);
}

int afsk_file_sizes(const char* const* paths, int32_t n_files, int64_t* out_size_bytes) {
    if (n_files < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_files == 0) return AFSK_OK;
    if (!paths || !out_size_bytes) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    for (int32_t i = 0; i < n_files; i++)
        if (!paths[i]) return fail(AFSK_E_INVALID_ARG, "null path");
    return no_throw([&] {
        io_pool().run((size_t)n_files, io_threads(), [&](size_t i) {
            struct stat st;
            out_size_bytes[i] = stat(paths[i], &st) == 0 ? (int64_t)st.st_size : -1;
        });
        return AFSK_OK;
    });
}

// afsk_wav_ingest: ONE pass per file -- open, header walk, pread of the data chunk straight into pinned
// memory, close -- pipelined against the H2D copies through a RingSession: windows of whole slots (a gap of more
// than kGapFill bytes between two slots ends a window), pool threads fill the pieces in order, the calling thread
// sends window w when its last piece is in, and window w + slots may be filled once the copy of window w has completed.
static int wav_ingest_impl(const char* const* paths, int32_t n_files, const int64_t* slot_offset,
                           const int64_t* slot_samples, int16_t* d_samples, int64_t capacity_samples,
                           int64_t* out_data_offset, int64_t* out_data_bytes, int32_t* out_status) {
    if (n_files < 0 || capacity_samples < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_files == 0) return AFSK_OK;
    if (!paths || !slot_offset || !slot_samples || !d_samples || !out_data_offset || !out_data_bytes || !out_status)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const size_t n = (size_t)n_files;
    LayoutCheck layout{"slot", capacity_samples};
    for (size_t s = 0; s < n; s++)
        if (int rc0 = layout.next(paths[s] != nullptr, slot_offset[s], slot_samples[s])) return rc0;
    if (int rc0 = require_device()) return rc0;
    static const bool kStats = std::getenv("AFSK_INGEST_STATS") != nullptr;
    constexpr size_t kGapFill = 256;
    RingSession ring;
    if (int rc0 = ring.open()) return rc0;
    // (the sender zero-fills everything of a window that no piece covers: the gaps are part of what is delivered)
    ring.plan(n, [&](size_t s) { return (size_t)slot_offset[s] * 2; }, [&](size_t s) { return (size_t)slot_samples[s] * 2; },
              kGapFill, /*gaps_delivered=*/true);
    const auto& pieces = ring.pieces; const auto& wins = ring.wins;
    const size_t nwin = wins.size(), npieces = pieces.size();
    ring.open_through(RingSession::slots());              // the windows whose staging buffer may be filled
    // stats (AFSK_INGEST_STATS): nanoseconds summed over the fillers / spent by the sender
    std::atomic<long long> ns_wait_release{0}, ns_open{0}, ns_read{0}, ns_close{0}, n_fast{0};
    long long ns_wait_fill = 0, ns_wait_sent = 0, ns_issue = 0;
    auto now_ns = [] { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                           std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const long long t_begin = now_ns();

    auto fill_piece = [&](size_t i) {
        const StagePiece& pc = pieces[i];
        const long long t_wait = kStats ? now_ns() : 0;
        ring.wait_open(pc.win);
        if (kStats) ns_wait_release.fetch_add(now_ns() - t_wait, std::memory_order_relaxed);
        char* dst = ring.buffer(pc.win) + pc.stage_off;
        if (!ring.failed()) {
            int64_t doff = 0, dbytes = 0;
            int st = AFSK_WAV_IO;
            long long t0 = kStats ? now_ns() : 0;
            const int fd = open(paths[pc.file], O_RDONLY | O_CLOEXEC);
            if (kStats) { const long long t1 = now_ns(); ns_open.fetch_add(t1 - t0, std::memory_order_relaxed); t0 = t1; }
            const size_t cap = (size_t)slot_samples[pc.file] * 2;
            bool have_data = false;
            // The common file -- a canonical 44-byte header (wav_canonical_data) whose whole data chunk is this
            // one piece -- is read with ONE preadv: header into a local buffer, data straight into the staging
            // slot.  Anything else (more chunks, odd sizes, a piece of a split slot) takes the general walk below.
            if (fd >= 0 && pc.lo == 0 && pc.bytes == cap && cap > 0) {
                unsigned char hdr[44];
                struct iovec iov[2] = {{hdr, sizeof hdr}, {dst, cap}};
                const ssize_t got = preadv(fd, iov, 2, 0);
                struct stat sb;
                // the read is trusted only if it returned everything the file holds up to the end of the slot
                // (a short read that is not the end of the file -- POSIX allows it -- takes the general walk)
                if (got >= 44 && fstat(fd, &sb) == 0 &&
                    (int64_t)got == std::min<int64_t>((int64_t)sb.st_size, 44 + (int64_t)cap) &&
                    wav_canonical_data(hdr, (int64_t)sb.st_size, &dbytes)) {
                    doff = 44;
                    const size_t usable = (size_t)dbytes & ~(size_t)1;
                    if (usable <= cap && 44 + (int64_t)usable <= (int64_t)got) {
                        st = AFSK_WAV_OK;
                        have_data = true;
                        out_data_offset[pc.file] = doff; out_data_bytes[pc.file] = dbytes; out_status[pc.file] = st;
                        if (cap > usable) std::memset(dst + usable, 0, cap - usable);   // rest of the slot: zeros
                        if (kStats) n_fast.fetch_add(1, std::memory_order_relaxed);
                    }
                }
            }
            if (!have_data) {
                if (fd >= 0) st = wav_probe_fd(fd, &doff, &dbytes);
                size_t usable = st == AFSK_WAV_OK ? ((size_t)dbytes & ~(size_t)1) : 0;
                if (usable > cap) { st = AFSK_WAV_SLOT; usable = 0; }          // the caller's slot is too small: left to the caller
                if (pc.lo == 0) { out_data_offset[pc.file] = doff; out_data_bytes[pc.file] = dbytes; out_status[pc.file] = st; }
                const size_t lo = std::min(usable, pc.lo), hi = std::min(usable, pc.lo + pc.bytes);
                size_t have = hi > lo ? hi - lo : 0;
                // a file that shrank between the walk and the read is that FILE's problem, not the batch's:
                // zeroed slot, status AFSK_WAV_IO, the caller's fallback reader reports it
                if (have > 0 && !pread_all(fd, dst, have, doff + (int64_t)lo)) { out_status[pc.file] = AFSK_WAV_IO; have = 0; }
                if (pc.bytes > have) std::memset(dst + have, 0, pc.bytes - have);   // rest of the slot: zeros
            }
            if (kStats) { const long long t1 = now_ns(); ns_read.fetch_add(t1 - t0, std::memory_order_relaxed); t0 = t1; }
            if (fd >= 0) close(fd);
            if (kStats) ns_close.fetch_add(now_ns() - t0, std::memory_order_relaxed);
        }
        ring.piece_done(pc.win);
    };

    // when the last piece of window w is in, the coordinator sends the window; window w + slots may be filled once
    // the copy of window w has completed
    const int rc = ring.run(fill_piece, [&](auto&& serial_through) {
        size_t gap_scan = 0;
        for (size_t w = 0; w < nwin && ring.ok(); w++) {
            serial_through(w);
            const long long t0 = kStats ? now_ns() : 0;
            ring.wait_done(w);
            const long long t1 = kStats ? now_ns() : 0;
            ns_wait_fill += t1 - t0;
            char* st = ring.buffer(w);
            // gaps of up to kGapFill bytes between two slots of the window travel with it as zeros
            size_t cur = 0;
            for (; gap_scan < npieces && pieces[gap_scan].win <= w; gap_scan++) {   // pieces are in window order
                const StagePiece& pc = pieces[gap_scan];
                if (pc.win != w || pc.bytes == 0) continue;
                if (pc.stage_off > cur) std::memset(st + cur, 0, pc.stage_off - cur);
                cur = std::max(cur, pc.stage_off + pc.bytes);
            }
            if (cur < wins[w].bytes) std::memset(st + cur, 0, wins[w].bytes - cur);   // (a window that is all gap)
            // windows alternate between two copy streams (disjoint device ranges: no order needed between them),
            // so the next transfer is already queued when one ends
            if (wins[w].bytes > 0 &&
                !ring.hip(hipMemcpyAsync((char*)d_samples + wins[w].dev_b0, st, wins[w].bytes, hipMemcpyHostToDevice,
                                         ring.stream(w)), "H2D samples"))
                break;
            if (!ring.hip(hipEventRecord(ring.event(w), ring.stream(w)), "hipEventRecord")) break;
            const long long t2 = kStats ? now_ns() : 0;
            if (kStats) ns_issue += t2 - t1;
            // keep two transfers queued: only when window w - 1 has left its staging buffer is that buffer handed
            // to the fillers of window w - 1 + slots
            if (w >= 1) {
                ring.hip(hipEventSynchronize(ring.event(w - 1)), "hipEventSynchronize");
                if (kStats) ns_wait_sent += now_ns() - t2;
                ring.open_through(w + RingSession::slots());
            }
        }
    });
    if (kStats) {
        const double ms = 1e-6;
        std::fprintf(stderr, "afsk_wav_ingest: %zu files, %zu windows of %zu MiB x %zu slots, %u fillers, %.2f ms total | sender: "
                     "wait-filled %.2f issue %.2f wait-sent %.2f ms | fillers (sum over threads): wait-release %.2f open %.2f "
                     "read %.2f close %.2f ms, one-preadv files %lld\n", n, nwin, RingSession::window_bytes() >> 20,
                     RingSession::slots(), ring.width(),
                     (now_ns() - t_begin) * ms, ns_wait_fill * ms, ns_issue * ms, ns_wait_sent * ms,
                     ns_wait_release.load() * ms, ns_open.load() * ms, ns_read.load() * ms, ns_close.load() * ms,
                     (long long)n_fast.load());
    }
    return rc;
}

int afsk_wav_ingest(const char* const* paths, int32_t n_files, const int64_t* slot_offset,
                    const int64_t* slot_samples, int16_t* d_samples, int64_t capacity_samples,
                    int64_t* out_data_offset, int64_t* out_data_bytes, int32_t* out_status) {
    return afsk::guarded(wav_ingest_impl, paths, n_files, slot_offset, slot_samples, d_samples, capacity_samples,
                         out_data_offset, out_data_bytes, out_status);
}

// ---- .wav egress at scale: device streams -> canonical RIFF/WAVE files (Transmitter.save for many payloads) ----
// The mirror image of afsk_wav_ingest: the calling thread copies windows of the device range into the pinned
// staging ring (D2H, two alternating streams) and hands every window to the pool as soon as its copy has
// completed; pool threads write the file pieces of the window -- one open / pwritev (header + data) / close for a
// file that lies inside one window -- and a staging buffer is reused once all its pieces are on their way.
static int wav_egress_impl(const char* const* paths, int32_t n_files, const int16_t* d_samples,
                           const int64_t* stream_offset, const int32_t* stream_len, int32_t* out_status) {
    if (n_files < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_files == 0) return AFSK_OK;
    if (!paths || !d_samples || !stream_offset || !stream_len || !out_status)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    const size_t n = (size_t)n_files;
    LayoutCheck layout{"stream", std::numeric_limits<int64_t>::max()};
    for (size_t s = 0; s < n; s++) {
        if (int rc0 = layout.next(paths[s] != nullptr, stream_offset[s], stream_len[s])) return rc0;
        if ((int64_t)stream_len[s] > (int64_t)((0xFFFFFFFFll - 36) / 2))
            return fail(AFSK_E_INVALID_ARG, "a stream too long for a RIFF file");
    }
    if (int rc0 = require_device()) return rc0;
    RingSession ring;
    if (int rc0 = ring.open()) return rc0;
    // windows over the device byte range; a gap of more than 64 KiB between two streams is not copied (a smaller one
    // is copied along inside a window and written nowhere: no part of what is delivered)
    constexpr size_t kGapCopy = (size_t)64 << 10;
    ring.plan(n, [&](size_t s) { return (size_t)stream_offset[s] * 2; }, [&](size_t s) { return (size_t)stream_len[s] * 2; },
              kGapCopy, /*gaps_delivered=*/false);
    const auto& pieces = ring.pieces; const auto& wins = ring.wins;
    const size_t nwin = wins.size(), slots = RingSession::slots();
    for (size_t s = 0; s < n; s++) out_status[s] = AFSK_WAV_OK;

    auto write_piece = [&](size_t i) {
        const StagePiece& pc = pieces[i];
        ring.wait_open(pc.win);                                   // open = its D2H copy has completed
        if (!ring.failed()) {
            const uint32_t total = (uint32_t)stream_len[pc.file] * 2u;
            const bool whole = pc.lo == 0 && pc.bytes == total;   // the file lies inside one window
            // No O_TRUNC: an existing file is overwritten IN PLACE (its page-cache pages are reused instead of freed and
            // allocated again) and every piece sets the final size -- the pieces of a file that spans windows are
            // written concurrently, in any order, and ftruncate to the size a file already has costs nothing.
            const int fd = open(paths[pc.file], O_WRONLY | O_CREAT | O_CLOEXEC, 0666);
            bool ok = fd >= 0;
            if (ok && !whole) ok = ftruncate(fd, (off_t)(44 + (int64_t)total)) == 0;
            if (ok) {
                unsigned char hdr[44];
                struct iovec iov[2];
                int niov = 0;
                int64_t off = 44 + (int64_t)pc.lo;
                if (pc.lo == 0) { wav_canonical_header(hdr, total); iov[niov++] = {hdr, sizeof hdr}; off = 0; }
                if (pc.bytes > 0) iov[niov++] = {ring.buffer(pc.win) + pc.stage_off, pc.bytes};
                size_t want = (pc.lo == 0 ? 44 : 0) + pc.bytes;
                while (ok && want > 0) {                          // pwritev may be partial
                    const ssize_t r = pwritev(fd, iov, niov, (off_t)off);
                    if (r <= 0) { ok = false; break; }
                    want -= (size_t)r; off += r;
                    size_t adv = (size_t)r;
                    while (adv > 0 && niov > 0) {
                        if (adv >= iov[0].iov_len) { adv -= iov[0].iov_len; iov[0] = iov[1]; niov--; }
                        else { iov[0].iov_base = (char*)iov[0].iov_base + adv; iov[0].iov_len -= adv; adv = 0; }
                    }
                }
            }
            if (ok && whole) ok = ftruncate(fd, (off_t)(44 + (int64_t)total)) == 0;   // (an existing longer file)
            if (fd >= 0 && close(fd) != 0) ok = false;
            if (!ok) out_status[pc.file] = AFSK_WAV_IO;           // that file's problem; the batch goes on
        }
        ring.piece_done(pc.win);
    };

    return ring.run(write_piece, [&](auto&& serial_through) {
        size_t issued = 0;
        for (size_t w = 0; w < nwin && ring.ok(); w++) {
            while (issued < nwin && issued < w + slots) {         // keep copies ahead of the writers, one per free buffer
                if (issued >= slots) {
                    const size_t dep = issued - slots;            // the window whose buffer this copy reuses (dep < w: open)
                    if (!ring.window_done(dep)) {
                        if (issued > w) break;                    // window w itself is on its way: look again later
                        serial_through(dep);
                        ring.wait_done(dep);
                    }
                }
                if (wins[issued].bytes > 0 &&
                    !ring.hip(hipMemcpyAsync(ring.buffer(issued), (const char*)d_samples + wins[issued].dev_b0,
                                             wins[issued].bytes, hipMemcpyDeviceToHost, ring.stream(issued)), "D2H samples"))
                    break;
                if (!ring.hip(hipEventRecord(ring.event(issued), ring.stream(issued)), "hipEventRecord")) break;
                issued++;
            }
            if (!ring.ok() || !ring.hip(hipEventSynchronize(ring.event(w)), "hipEventSynchronize")) break;
            ring.open_through(w + 1);                             // window w has landed: its pieces may be written
            serial_through(w);
        }
    });
}

int afsk_wav_egress(const char* const* paths, int32_t n_files, const int16_t* d_samples,
                    const int64_t* stream_offset, const int32_t* stream_len, int32_t* out_status) {
    return afsk::guarded(wav_egress_impl, paths, n_files, d_samples, stream_offset, stream_len, out_status);
}

int afsk_modulate_batch(const uint8_t* payload, int32_t payload_stride,
                        const int32_t* payload_len, const int32_t* bit_frames,
                        const int32_t* ts_cycles, const int64_t* stream_offset,
                        const int32_t* stream_len, int32_t max_stream_len, int32_t n_streams,
                        int32_t wav_quirk, int16_t* samples, void* hip_stream) {
    if (n_streams < 0 || payload_stride < 0 || max_stream_len < 0)
        return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0 || max_stream_len == 0) return AFSK_OK;
    if (!payload_len || !bit_frames || !ts_cycles || !stream_offset || !stream_len || !samples ||
        (!payload && payload_stride > 0))
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    afsk::ModulateArgs a;
    a.payload = payload; a.payload_stride = payload_stride; a.payload_len = payload_len;
    a.bit_frames = bit_frames; a.ts_cycles = ts_cycles; a.stream_offset = stream_offset;
    a.stream_len = stream_len; a.n_streams = n_streams; a.wav_quirk = wav_quirk;
    a.samples = samples; a.chunks = 0;
    hipError_t e = afsk::launch_modulate(a, max_stream_len, (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch modulate_kernel");
}

static int gate_batch_impl(const int16_t* samples, const int64_t* stream_offset,
                           const int32_t* stream_len, int32_t max_stream_len,
                           int32_t amp_start_threshold, int32_t amp_end_threshold, int32_t n_streams,
                           int32_t max_bursts, int32_t* block_amp, int32_t* out_n_bursts,
                           int32_t* out_burst_start, int32_t* out_burst_len, int32_t* out_open_end,
                           int64_t* out_slot_offset, int32_t* out_slot_len, void* hip_stream) {
    if (n_streams < 0 || max_stream_len < 0 || max_bursts < 0)
        return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0) return AFSK_OK;
    const int32_t max_blocks = max_stream_len / 2048;
    if (!samples || !stream_offset || !stream_len || !out_n_bursts || !out_open_end ||
        (max_blocks > 0 && !block_amp) || (max_bursts > 0 && (!out_burst_start || !out_burst_len)))
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if ((out_slot_offset == nullptr) != (out_slot_len == nullptr))
        return fail(AFSK_E_INVALID_ARG, "out_slot_offset and out_slot_len go together");
    if (int rc = require_device()) return rc;
    afsk::GateArgs a;
    a.samples = samples; a.stream_offset = stream_offset; a.stream_len = stream_len;
    a.amp_start = amp_start_threshold; a.amp_end = amp_end_threshold; a.n_streams = n_streams;
    a.max_len = max_stream_len;
    a.max_blocks = max_blocks; a.max_bursts = max_bursts; a.block_amp = block_amp;
    a.out_n_bursts = out_n_bursts; a.out_burst_start = out_burst_start;
    a.out_burst_len = out_burst_len; a.out_open_end = out_open_end;
    a.out_slot_offset = max_bursts > 0 ? out_slot_offset : nullptr;
    a.out_slot_len = max_bursts > 0 ? out_slot_len : nullptr;
    hipError_t e = afsk::launch_gate(a, (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch gate kernels");
}

int afsk_gate_batch(const int16_t* samples, const int64_t* stream_offset,
                    const int32_t* stream_len, int32_t max_stream_len,
                    int32_t amp_start_threshold, int32_t amp_end_threshold, int32_t n_streams,
                    int32_t max_bursts, int32_t* block_amp, int32_t* out_n_bursts,
                    int32_t* out_burst_start, int32_t* out_burst_len, int32_t* out_open_end,
                    void* hip_stream) {
    return gate_batch_impl(samples, stream_offset, stream_len, max_stream_len, amp_start_threshold, amp_end_threshold,
                           n_streams, max_bursts, block_amp, out_n_bursts, out_burst_start, out_burst_len, out_open_end,
                           nullptr, nullptr, hip_stream);
}

int afsk_gate_batch_slots(const int16_t* samples, const int64_t* stream_offset,
                          const int32_t* stream_len, int32_t max_stream_len,
                          int32_t amp_start_threshold, int32_t amp_end_threshold, int32_t n_streams,
                          int32_t max_bursts, int32_t* block_amp, int32_t* out_n_bursts,
                          int32_t* out_burst_start, int32_t* out_burst_len, int32_t* out_open_end,
                          int64_t* out_slot_offset, int32_t* out_slot_len, void* hip_stream) {
    if (max_bursts > 0 && (!out_slot_offset || !out_slot_len)) return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    return gate_batch_impl(samples, stream_offset, stream_len, max_stream_len, amp_start_threshold, amp_end_threshold,
                           n_streams, max_bursts, block_amp, out_n_bursts, out_burst_start, out_burst_len, out_open_end,
                           out_slot_offset, out_slot_len, hip_stream);
}

int afsk_add_noise_batch(int16_t* samples, const int64_t* stream_offset,
                         const int32_t* stream_len, int32_t max_stream_len,
                         const int32_t* scale_q24, int32_t n_streams, uint32_t seed,
                         uint32_t stream_idx_base, void* hip_stream) {
    if (n_streams < 0 || max_stream_len < 0) return fail(AFSK_E_INVALID_ARG, "negative size");
    if (n_streams == 0 || max_stream_len == 0) return AFSK_OK;
    if (!samples || !stream_offset || !stream_len || !scale_q24)
        return fail(AFSK_E_INVALID_ARG, "null pointer argument");
    if (int rc = require_device()) return rc;
    afsk::NoiseArgs a;
    a.samples = samples; a.stream_offset = stream_offset; a.stream_len = stream_len;
    a.scale_q24 = scale_q24; a.n_streams = n_streams; a.seed = seed;
    a.stream_idx_base = stream_idx_base; a.chunks = 0;
    hipError_t e = afsk::launch_noise(a, max_stream_len, (hipStream_t)hip_stream);
    return e == hipSuccess ? AFSK_OK : hip_fail(e, "launch noise_kernel");
}

}  // extern "C"
