// afsk_host_plan.h -- the rate-grouped dispatch plan of a mixed-baud batch and the launch choice of the host
// entries.  Host code only, included by afsk_capi.hip alone (everything here has internal linkage).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "afsk_capi_internal.h"
#include "afsk_kernels.h"

namespace {

// ---- rate-grouped dispatch of a mixed-baud batch (afsk_demod_batch_grouped) -----------------------------
// The host can see bit_frames: the streams are bucketed by value and the batch is decoded by ONE launch of the
// per-stream kernel (every geometry a Receiver can have is compiled into it) that walks the streams BUCKET BY
// BUCKET through an index list, so that the waves resident on a CU at any time run the same geometry's code
// (wave w decodes stream index[w]; every per-stream array stays indexed by the stream number).
// Measured alternatives (profiles/archive/r4_exp2_grouped_modes.txt): one launch of the uniform kernel per bucket --
// on side streams forked / joined with events, or one after the other -- loses 2 ... 70 % to the cross-queue
// hand-over (~27 us per step) and to kernels of different queues hardly overlapping on gfx950
// (hipExtAnyOrderLaunch is not honoured there); the rate-sorted single launch gains 3 ... 12 % over stream
// order when four or more rates are mixed and loses 2 % with three (config #3), hence kSortFromGroups.
struct GroupPlan {
    struct Group { int32_t bf; int32_t first; int32_t count; };
    static constexpr size_t kSortFromGroups = 4;  // fewer distinct rates: stream order (no index list)
    int device = -1;
    int32_t n = 0;
    std::vector<Group> groups;                   // valid rates, largest bucket first; then bf 0: the refused streams
    std::vector<int32_t> h_upload;               // [n] index list (bucket after bucket) + [n] bit_frames by stream number
    int32_t* d_index = nullptr;                  // [n] the permutation; followed, in the same storage, by
    int32_t* d_bf = nullptr;                     // [n] bit_frames by stream number (the kernel's per-stream switch reads it)
    bool own_index = false;
    bool by_length = false;                      // r6: inside every window and bucket the longest streams come first

    ~GroupPlan() {
        if (own_index && d_index) (void)hipFree(d_index);
    }

    bool sorted() const { return by_length || groups.size() >= sort_from(); }
    static size_t sort_from() {                  // AFSK_GROUP_SORT_FROM overrides (A/B runs)
        const char* e = std::getenv("AFSK_GROUP_SORT_FROM");
        return (e && *e) ? (size_t)std::atol(e) : kSortFromGroups;
    }

    // Ragged batches (r6).  One wavefront decodes one stream whatever its length, and the four wavefronts of a
    // workgroup share its LDS allocation: a workgroup holds its quarter of a CU until its LONGEST stream ends, so four
    // neighbours of 0.25 / 0.25 / 0.25 / 4 s keep three wave slots idle for most of the group's life, and the launch ends
    // when the last long stream does.  With the stream lengths visible to the host (h_len) the walk therefore takes,
    // inside every window and rate bucket, the longest streams first (stable: equal lengths keep stream order) -- the
    // four streams of a workgroup are then neighbours in length, and what a window dispatches last is short.  Only when
    // the lengths differ enough to matter: the shortest stream below 3/4 of the longest (a batch of equal lengths keeps
    // its stream order and, with one rate, its plain uniform launch).
    static bool lengths_ragged(const int32_t* h_len, int32_t n_streams) {
        if (!h_len || n_streams < 8) return false;
        int32_t lo = h_len[0], hi = h_len[0];
        for (int32_t s = 1; s < n_streams; s++) { lo = std::min(lo, h_len[s]); hi = std::max(hi, h_len[s]); }
        return hi > 0 && (int64_t)lo * 4 < (int64_t)hi * 3;
    }

    // host part: buckets and permutation (stable inside a bucket: ascending stream number)
    void bucket(const int32_t* h_bf, int32_t n_streams, const int32_t* h_len = nullptr) {
        n = n_streams;
        by_length = lengths_ragged(h_len, n_streams) && !std::getenv("AFSK_GROUP_NO_LENGTH_SORT");
        std::vector<int32_t> count(AFSK_SYNC_WINDOW / 2 + 1, 0);    // slot 0 = every invalid value
        auto slot = [](int32_t bf) { return afsk::bf_valid(bf) ? bf : 0; };
        for (int32_t s = 0; s < n; s++) count[(size_t)slot(h_bf[s])]++;
        std::vector<int32_t> order;
        for (int32_t bf = 4; bf < (int32_t)count.size(); bf += 4)
            if (count[(size_t)bf]) order.push_back(bf);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return count[(size_t)a] > count[(size_t)b]; });
        if (count[0]) order.push_back(0);
        std::vector<int32_t> cursor(count.size(), 0);
        int32_t first = 0;
        for (int32_t bf : order) {
            groups.push_back({bf, first, count[(size_t)bf]});
            cursor[(size_t)bf] = first;
            first += count[(size_t)bf];
        }
        h_upload.resize(2 * (size_t)n);
        // (ragged batches walk windows twice as long: 8192 streams measured best -- time per byte against 1 s streams
        // 1.06 / 1.03 / 1.00 / 1.01 / 1.02 for windows of 2048 / 4096 / 8192 / 16384 / the whole batch,
        // profiles/r6_ragged_windows.txt -- the longest streams of a window live several generations of short ones)
        const int32_t window = by_length && !std::getenv("AFSK_GROUP_WINDOW") ? 2 * sort_window() : sort_window();
        // longest first inside [b, e) of the index list (one bucket of one window)
        auto by_len = [&](size_t b, size_t e) {
            if (by_length && e - b > 1)
                std::stable_sort(h_upload.begin() + (ptrdiff_t)b, h_upload.begin() + (ptrdiff_t)e,
                                 [&](int32_t x, int32_t y) { return h_len[x] > h_len[y]; });
        };
        if (window <= 0 || window >= n) {
            for (int32_t s = 0; s < n; s++) h_upload[(size_t)cursor[(size_t)slot(h_bf[s])]++] = s;
            for (const Group& g : groups) by_len((size_t)g.first, (size_t)g.first + (size_t)g.count);
        } else {
            // bucket order INSIDE windows of `window` consecutive streams (see sort_window)
            std::vector<int32_t> wc(count.size());
            size_t at = 0;
            for (int32_t w0 = 0; w0 < n; w0 += window) {
                const int32_t w1 = std::min(n, w0 + window);
                std::fill(wc.begin(), wc.end(), 0);
                for (int32_t s = w0; s < w1; s++) wc[(size_t)slot(h_bf[s])]++;
                size_t run = at;
                for (int32_t bf : order) { cursor[(size_t)bf] = (int32_t)run; run += (size_t)wc[(size_t)bf]; }
                for (int32_t s = w0; s < w1; s++) h_upload[(size_t)cursor[(size_t)slot(h_bf[s])]++] = s;
                run = at;
                for (int32_t bf : order) { by_len(run, run + (size_t)wc[(size_t)bf]); run += (size_t)wc[(size_t)bf]; }
                at = run;
            }
        }
        if (n > 0) std::memcpy(h_upload.data() + n, h_bf, (size_t)n * 4);
    }

    // The walk visits the buckets one after the other INSIDE windows of this many consecutive streams (r5; 0 = over
    // the whole batch, r4's form).  The 2048 streams in flight of a walk over the whole batch are spread over as many
    // times the address range as there are rates cycling over the streams, and that alone costs 3.5 - 5 % (one rate
    // read in that order: profiles/r5_exp37_address_order.txt).  Windows of 4096 streams -- two generations of
    // resident wavefronts -- keep the streams in flight within 0.4 GB and the neighbouring wavefronts on one rate's
    // code: -2.8 % for four cycling rates, -2.2 % for eighteen, unchanged at 4096 streams (1024: -3.7 / -3.1 % but
    // +2 % at 4096 streams; profiles/r5_exp38_windowed_walk.txt).  AFSK_GROUP_WINDOW overrides (A/B runs).
    static int32_t sort_window() {
        const char* e = std::getenv("AFSK_GROUP_WINDOW");
        if (e && *e) return (int32_t)std::atol(e);
        return 4096;
    }

    // device part: index list + bit_frames either in storage the caller provides (2 n int32, copied
    // asynchronously on `copy_stream`, which every launch of this plan must follow) or in an allocation of its
    // own (copied synchronously)
    hipError_t materialise(int32_t* index_storage, hipStream_t copy_stream) {
        hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess || n == 0) return e;
        if (index_storage) {
            d_index = index_storage;
            d_bf = d_index + n;
            return hipMemcpyAsync(d_index, h_upload.data(), (size_t)n * 8, hipMemcpyHostToDevice, copy_stream);
        }
        e = hipMalloc((void**)&d_index, (size_t)n * 8);
        if (e != hipSuccess) { d_index = nullptr; return e; }
        d_bf = d_index + n;
        own_index = true;
        return hipMemcpy(d_index, h_upload.data(), (size_t)n * 8, hipMemcpyHostToDevice);
    }

    // ONE launch: the uniform kernel when the whole batch is one valid rate, else the per-stream kernel
    // (in bucket order from kSortFromGroups rates on); a stream with an invalid bit_frames gets status 3 from
    // the kernel itself.  Nothing but a kernel launch: asynchronous, capture-safe, no state shared between calls.
    hipError_t launch(afsk::DemodArgs a, hipStream_t stream) const {
        a.n_streams = n;
        if (groups.size() == 1 && groups[0].bf > 0) {
            a.bit_frames = nullptr;
            a.uniform_bit_frames = groups[0].bf;
            a.stream_index = by_length ? d_index : nullptr;      // one rate, ragged lengths: the uniform kernel walks the list
            return afsk::launch_demod_uniform(a, stream);
        }
        a.bit_frames = d_bf;
        a.stream_index = sorted() ? d_index : nullptr;
        return afsk::launch_demod(a, stream);
    }
};

// The host entries see the bit_frames array (checked valid, the device present): one value for all streams ->
// the uniform kernel; several -> the grouped dispatch (index list + bit_frames live in `index_storage`, 2 n int32 of
// the caller's device scratch; `keep` owns the plan's host side until the caller has synchronised).
int demod_device_auto(const int32_t* h_bit_frames, const int32_t* h_stream_len, const int16_t* samples,
                      const int64_t* stream_offset, const int32_t* stream_len, int32_t amp_end_threshold,
                      int32_t n_streams, const afsk::DemodOutputs& o, hipStream_t stream, int32_t* index_storage,
                      std::unique_ptr<GroupPlan>& keep) {
    afsk::DemodArgs a = o.args<afsk::DemodArgs>(samples, stream_offset, stream_len, amp_end_threshold, n_streams);
    bool same = true;
    for (int32_t s = 1; s < n_streams && same; s++) same = h_bit_frames[s] == h_bit_frames[0];
    // (one rate but ragged lengths: the plan, whose walk takes the longest streams first -- GroupPlan::bucket)
    if (same && !GroupPlan::lengths_ragged(h_stream_len, n_streams)) {
        a.uniform_bit_frames = h_bit_frames[0];
        hipError_t e = afsk::launch_demod_uniform(a, stream);
        return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch demod_uniform_kernel");
    }
    keep.reset(new GroupPlan());
    keep->bucket(h_bit_frames, n_streams, h_stream_len);
    hipError_t e = keep->materialise(index_storage, stream);
    if (e != hipSuccess) return afsk::hip_fail(e, "grouped dispatch (index list)");
    e = keep->launch(a, stream);
    return e == hipSuccess ? AFSK_OK : afsk::hip_fail(e, "launch demod_kernel (grouped)");
}

}  // namespace
