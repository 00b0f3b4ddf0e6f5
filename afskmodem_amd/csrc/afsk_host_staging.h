// afsk_host_staging.h -- how the host entries move bytes between host memory or files and the device: the cached
// device scratch with its pinned staging buffers (ScratchLease), the per-thread copy streams, the layout check of
// the file entries, the two-window loop of the gather and upload entries, and the window planner and ring session
// of the one-pass file entries (afsk_wav_ingest, afsk_wav_egress).  Host code only, included by afsk_capi.hip alone
// (everything here has internal linkage).
#pragma once

#include <limits>
#include <memory>

#include "afsk_capi_internal.h"
#include "afsk_host_pool.h"   // (and the standard headers it includes)

namespace {

using afsk::fail;
using afsk::hip_fail;

// Device scratch of the host-buffer entry, kept between calls: hipMalloc of a few hundred MB
// costs tens of ms (75 ms for 393 MB measured, tools/h2d_probe), far more than the transfer.
// One cached allocation per process, grown on demand; a concurrent caller that finds it busy
// falls back to a private hipMalloc/hipFree.  afsk_host_scratch_release() frees it.
constexpr size_t kStageBytes = (size_t)32 << 20;   // pinned staging window of the gather entry

struct ScratchCache {
    std::mutex mu;
    char* ptr = nullptr;
    size_t cap = 0;
    int device = -1;
    char* stage[2] = {nullptr, nullptr};            // pinned host windows (afsk_demod_streams_host)
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    // the file entries' staging ring: chunks 0 and 1 ARE stage[0] / stage[1]; 2 and 3 are allocated the first
    // time a ring of more than 64 MiB is asked for; one event per ring slot
    char* ring_extra[2] = {nullptr, nullptr};
    hipEvent_t ring_sent[16] = {};
};
constexpr size_t kRingChunks = 4;
constexpr int kMaxRingSlots = 16;
ScratchCache g_scratch;

class ScratchLease {
public:
    ~ScratchLease() {
        if (private_ptr_) (void)hipFree(private_ptr_);
        if (locked_) g_scratch.mu.unlock();
    }
    // block = wait for the shared cache instead of falling back to a private allocation
    hipError_t acquire(size_t bytes, char** out, bool block = false) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (block) g_scratch.mu.lock();
        if (block || g_scratch.mu.try_lock()) {
            locked_ = true;
            if (g_scratch.cap < bytes || g_scratch.device != dev) {
                if (g_scratch.ptr) (void)hipFree(g_scratch.ptr);
                g_scratch.ptr = nullptr;
                g_scratch.cap = 0;
                if (g_scratch.device != dev) {
                    // events belong to the device they were created on: a cache that moves to
                    // another device drops them (staging() recreates them there); the pinned
                    // windows are hipHostMallocPortable and stay
                    for (int k = 0; k < 2; k++)
                        if (g_scratch.stage_free[k]) {
                            (void)hipEventDestroy(g_scratch.stage_free[k]);
                            g_scratch.stage_free[k] = nullptr;
                        }
                    for (hipEvent_t& ev : g_scratch.ring_sent)
                        if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
                }
                const size_t want = (bytes + (bytes >> 3) + ((size_t)2 << 20)) & ~(((size_t)2 << 20) - 1);
                e = hipMalloc((void**)&g_scratch.ptr, want);
                if (e != hipSuccess) { g_scratch.ptr = nullptr; return e; }
                g_scratch.cap = want;
                g_scratch.device = dev;
            }
            *out = g_scratch.ptr;
            return hipSuccess;
        }
        e = hipMalloc((void**)&private_ptr_, bytes);
        if (e != hipSuccess) { private_ptr_ = nullptr; return e; }
        *out = private_ptr_;
        return hipSuccess;
    }
    // The cache as a LOCK: the entries that need no device scratch of their own, only the pinned windows or the
    // ring, take a blocking lease of one byte -- whoever holds it owns the staging buffers until the lease ends.
    hipError_t lock() { char* d_unused = nullptr; return acquire(1, &d_unused, /*block=*/true); }
    // the two pinned staging windows (only with a blocking lease, which owns the cache)
    hipError_t staging(char* out_stage[2], hipEvent_t out_free[2]) {
        for (int k = 0; k < 2; k++) {
            if (!g_scratch.stage[k]) {
                NodeBinder on_the_devices_socket;
                hipError_t e = hipHostMalloc((void**)&g_scratch.stage[k], kStageBytes, hipHostMallocPortable);
                if (e != hipSuccess) { g_scratch.stage[k] = nullptr; return e; }
            }
            if (!g_scratch.stage_free[k]) {
                hipError_t e = hipEventCreateWithFlags(&g_scratch.stage_free[k], hipEventDisableTiming);
                if (e != hipSuccess) { g_scratch.stage_free[k] = nullptr; return e; }
            }
            out_stage[k] = g_scratch.stage[k]; out_free[k] = g_scratch.stage_free[k];
        }
        return hipSuccess;
    }
    // the file entries' ring of `slots` staging buffers of `window` bytes each (window divides 32 MiB,
    // slots * window <= 128 MiB) and one event per slot; only with a blocking lease
    hipError_t ring(size_t window, int slots, char** out_stage, hipEvent_t* out_sent) {
        char* chunk[kRingChunks] = {};
        hipEvent_t unused[2];
        hipError_t e = staging(chunk, unused);
        if (e != hipSuccess) return e;
        const size_t need = (size_t)slots * window;
        for (size_t c = 2; c < kRingChunks && c * kStageBytes < need; c++) {
            if (!g_scratch.ring_extra[c - 2]) {
                NodeBinder on_the_devices_socket;
                e = hipHostMalloc((void**)&g_scratch.ring_extra[c - 2], kStageBytes, hipHostMallocPortable);
                if (e != hipSuccess) { g_scratch.ring_extra[c - 2] = nullptr; return e; }
            }
        }
        chunk[2] = g_scratch.ring_extra[0]; chunk[3] = g_scratch.ring_extra[1];
        for (int k = 0; k < slots; k++) {
            const size_t o = (size_t)k * window;
            out_stage[k] = chunk[o / kStageBytes] + o % kStageBytes;
            if (!g_scratch.ring_sent[k]) {
                e = hipEventCreateWithFlags(&g_scratch.ring_sent[k], hipEventDisableTiming);
                if (e != hipSuccess) { g_scratch.ring_sent[k] = nullptr; return e; }
            }
            out_sent[k] = g_scratch.ring_sent[k];
        }
        return hipSuccess;
    }
private:
    bool locked_ = false;
    char* private_ptr_ = nullptr;
};

// The host-buffer entries run on a private NON-BLOCKING stream (one per calling thread and
// device, created on first use): on the NULL stream every call would synchronise implicitly with
// all other streams of the process -- the caller's own streams and other threads' calls.
struct ThreadStream {
    hipStream_t s = nullptr;
    int device = -1;
    ~ThreadStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t get(hipStream_t* out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (s && device != dev) { (void)hipStreamDestroy(s); s = nullptr; }
        if (!s) {
            e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
            if (e != hipSuccess) { s = nullptr; return e; }
            device = dev;
        }
        *out = s;
        return hipSuccess;
    }
};
thread_local ThreadStream g_thread_stream;
thread_local ThreadStream g_thread_stream2;      // a ring session alternates its copies between the two

// The layout rule of the file entries, one slot after the other: ascending, not overlapping, inside `capacity`
// samples.  `noun` ("stream" / "slot") is what the entry's interface calls them; end = where the last slot ended.
struct LayoutCheck {
    const char* noun;
    int64_t capacity, end = 0;
    int next(bool args_ok, int64_t offset, int64_t samples) {
        if (!args_ok || samples < 0 || offset < end)
            return fail(AFSK_E_INVALID_ARG, std::string(noun) + "s must be ascending and must not overlap");
        end = offset + samples;
        if (end > capacity) return fail(AFSK_E_INVALID_ARG, std::string(noun) + " outside the device buffer");
        return AFSK_OK;
    }
};

// The device byte range [b0, b1) through the lease's two pinned windows, one after the other: body(st, w0, w1) fills
// the pinned window `st` with what belongs at [w0, w1) and issues its copies on `stream` (returning a status) while
// the previous window is on the wire; a window is filled again once the copies recorded behind it have completed.
template <class Body>
int two_window_loop(ScratchLease& lease, hipStream_t stream, size_t b0, size_t b1, Body&& body) {
    char* stage[2];
    hipEvent_t stage_free[2];
    hipError_t e = lease.staging(stage, stage_free);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc (staging)");
    // small batches use smaller windows so that packing and DMA still overlap
    const size_t win = std::min(kStageBytes, std::max((size_t)1 << 20, (((b1 - b0) / 4) + 65535) & ~(size_t)65535));
    for (size_t w0 = b0, k = 0; w0 < b1; w0 += win, k++) {
        if (k >= 2 && (e = hipEventSynchronize(stage_free[k & 1])) != hipSuccess) return hip_fail(e, "hipEventSynchronize");
        if (int rc = body(stage[k & 1], w0, std::min(b1, w0 + win))) return rc;
        if ((e = hipEventRecord(stage_free[k & 1], stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    }
    return AFSK_OK;
}

// ---- the one-pass file entries: windows of slots through a ring of staging buffers --------------------------
// A piece is the part of slot `file` that lies in window `win`: `bytes` bytes from byte `lo` of the slot, at
// `stage_off` in the window's staging buffer.  An empty slot is one piece of 0 bytes.  Every piece's window exists.
struct StagePiece { size_t file; size_t win; size_t lo; size_t bytes; size_t stage_off; };
struct StageWindow { size_t dev_b0; size_t bytes; };

// Cuts n ascending slots (slot_b0(s) = device byte offset, slot_bytes(s) = size) into windows of whole slots where
// they fit; a slot larger than what is left of a window is split, a whole slot that merely does not fit the rest of
// the open window starts the next one.  A gap of more than `gap_limit` bytes between two slots ends a window; a
// smaller one lies inside it.  `gaps_delivered`: the gaps belong to what the windows deliver (the sender fills them),
// so a small gap behind a closed window becomes the head of the next one and a small gap in front of an empty slot
// extends the open window; without it a gap is carried along only between two pieces of one window.
template <class Off, class Size>
void plan_windows(size_t n, Off&& slot_b0, Size&& slot_bytes, size_t max_window, size_t gap_limit, bool gaps_delivered,
                  std::vector<StagePiece>& pieces, std::vector<StageWindow>& wins) {
    pieces.reserve(n + 8);
    size_t w_b0 = 0, w_b1 = 0;                    // open window's device byte range
    bool open_w = false;
    size_t last_end = 0;                          // device byte where the last closed window ended
    bool have_end = false;
    auto close_window = [&] {
        if (open_w) { wins.push_back({w_b0, w_b1 - w_b0}); open_w = false; last_end = w_b1; have_end = true; }
    };
    auto open_window = [&](size_t p0) {
        w_b0 = (gaps_delivered && have_end && p0 > last_end && p0 - last_end <= gap_limit) ? last_end : p0;
        w_b1 = p0;
        open_w = true;
    };
    // the first windows are SMALL (1, 2, 4 ... MiB up to the full window): the first transfer starts after a
    // fraction of a millisecond of file reading instead of after a whole 16 MiB of it
    auto win_cap = [&] { return std::min(max_window, ((size_t)1 << 20) << std::min<size_t>(wins.size(), 6)); };
    for (size_t s = 0; s < n; s++) {
        const size_t b0 = slot_b0(s), cap = slot_bytes(s);
        if (cap == 0) {                           // nothing to copy, but the slot still is a piece (a file to probe or write)
            // (an empty slot is a slot: a small gap in front of it travels like any other)
            if (gaps_delivered && open_w && b0 > w_b1 && b0 - w_b1 <= gap_limit && b0 - w_b0 <= win_cap()) w_b1 = b0;
            if (!open_w) open_window(b0);
            pieces.push_back({s, wins.size(), 0, 0, 0});
            continue;
        }
        size_t done = 0;
        while (done < cap) {
            const size_t p0 = b0 + done;
            if (open_w && (p0 > w_b1 + gap_limit || p0 - w_b0 >= win_cap())) close_window();
            if (!open_w) open_window(p0);
            const size_t wcap = win_cap();        // (closing a window may have moved on to a larger one)
            const size_t room = wcap - (p0 - w_b0);
            const size_t take = std::min(cap - done, room);
            // a whole slot that does not fit the rest of this window starts the next one
            if (take < cap - done && done == 0 && cap <= wcap && p0 != w_b0) { close_window(); continue; }
            pieces.push_back({s, wins.size(), done, take, p0 - w_b0});
            done += take;
            w_b1 = p0 + take;
            if (w_b1 - w_b0 >= wcap) close_window();
        }
    }
    close_window();
}

// What afsk_wav_ingest and afsk_wav_egress do around their loops.  Window w of the plan lives in staging buffer
// w % slots, has event w % slots and copies on stream w & 1.  Pool threads work the pieces off in order, the calling
// thread is the coordinator that issues the copies.  The hand-over between them goes through ONE mutex and two
// condition variables -- nobody spins: a pool thread sleeps until its piece's window is open to the pool (wait_open /
// open_through), and the one that finishes the last piece of a window wakes the coordinator (piece_done / wait_done).
class RingSession {
public:
    std::vector<StagePiece> pieces;
    std::vector<StageWindow> wins;
    // Staging ring of the file entries: slots() pinned buffers of window_bytes() each (default 8 x 16 MiB = the two
    // 32 MiB windows of the gather entry plus two more chunks allocated on first use; AFSK_INGEST_WINDOW_MB = 4 / 8 /
    // 16 / 32 and AFSK_INGEST_SLOTS = 2 ... 16 for experiments, at most 128 MiB in all).
    static size_t window_bytes() {
        static const int mb = [] { const char* e = std::getenv("AFSK_INGEST_WINDOW_MB"); return e ? std::atoi(e) : 16; }();
        return (size_t)((mb == 4 || mb == 8 || mb == 16 || mb == 32) ? mb : 16) << 20;
    }
    static size_t slots() {
        static const int want = [] { const char* e = std::getenv("AFSK_INGEST_SLOTS"); return e ? std::atoi(e) : 8; }();
        const int most = (int)std::min<size_t>((size_t)kMaxRingSlots, kRingChunks * kStageBytes / window_bytes());
        return (size_t)std::max(2, std::min(want, most));
    }
    // the pool on the device's socket, the calling thread's two copy streams, the cache's lock and the ring
    int open() {
        confine_pool_to_device_node();
        hipError_t e = g_thread_stream.get(&copy_stream_[0]);
        if (e == hipSuccess) e = g_thread_stream2.get(&copy_stream_[1]);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithFlags (host-entry streams)");
        if ((e = lease_.lock()) != hipSuccess) return hip_fail(e, "hipMalloc (host-entry scratch)");
        e = lease_.ring(window_bytes(), (int)slots(), stage_, event_);
        if (e != hipSuccess) return hip_fail(e, "hipHostMalloc / hipEventCreate (staging ring)");
        return AFSK_OK;
    }
    template <class Off, class Size>
    void plan(size_t n, Off&& slot_b0, Size&& slot_bytes, size_t gap_limit, bool gaps_delivered) {
        plan_windows(n, slot_b0, slot_bytes, window_bytes(), gap_limit, gaps_delivered, pieces, wins);
        remaining_.reset(new std::atomic<int>[std::max<size_t>(wins.size(), 1)]);
        for (size_t w = 0; w < wins.size(); w++) remaining_[w].store(0);
        for (const StagePiece& pc : pieces) remaining_[pc.win].fetch_add(1);
    }

    char* buffer(size_t w) const { return stage_[w % slots()]; }
    hipEvent_t event(size_t w) const { return event_[w % slots()]; }
    hipStream_t stream(size_t w) const { return copy_stream_[w & 1]; }
    // as many workers as can work on open windows at once, within the pool's size
    unsigned width() const { return (unsigned)std::min<size_t>(io_threads(), std::max<size_t>(1, pieces.size())); }

    // ---- pool threads
    void wait_open(size_t w) {                        // until window w is open to the pool (or the call has failed)
        std::unique_lock<std::mutex> lk(hand_mu_);
        cv_open_.wait(lk, [&] { return w < open_ || failed(); });
    }
    bool failed() const { return failed_.load(std::memory_order_relaxed) != 0; }
    void piece_done(size_t w) {
        if (remaining_[w].fetch_sub(1, std::memory_order_acq_rel) == 1) {
            std::lock_guard<std::mutex> lk(hand_mu_);     // last piece of the window: wake the coordinator
            cv_done_.notify_one();
        }
    }

    // ---- the coordinator
    void open_through(size_t count) {                 // windows [0, count) are open to the pool
        { std::lock_guard<std::mutex> lk(hand_mu_); open_ = count; }
        cv_open_.notify_all();
    }
    bool window_done(size_t w) const { return remaining_[w].load(std::memory_order_acquire) == 0; }
    void wait_done(size_t w) {                        // until every piece of window w is done
        std::unique_lock<std::mutex> lk(hand_mu_);
        cv_done_.wait(lk, [&] { return window_done(w) || failed(); });
    }
    bool hip(hipError_t e, const char* what) {        // notes the coordinator's first HIP error; false = stop issuing
        if (e != hipSuccess && herr_ == hipSuccess) { herr_ = e; hwhat_ = what; }
        return e == hipSuccess;
    }
    bool ok() const { return herr_ == hipSuccess; }

    // work(i) for every piece on the pool's threads while the caller runs coordinate(serial_through);
    // serial_through(w) works off, on the calling thread, the pieces of the windows up to w when the pool has no
    // thread to do it (and does nothing otherwise).  Afterwards nobody waits any more, both streams are synchronised
    // -- nothing may still use the staging buffers -- and a HIP error of either side is the return code.
    template <class Work, class Coordinate>
    int run(Work&& work, Coordinate&& coordinate) {
        const size_t npieces = pieces.size();
        io_pool().run_split(npieces, width(), work, [&](bool have_workers) {
            size_t next_serial = 0;
            auto serial_through = [&](size_t w) {
                while (!have_workers && next_serial < npieces && pieces[next_serial].win <= w) work(next_serial++);
            };
            coordinate(serial_through);
            if (!ok()) failed_.store(1);
            open_through(std::numeric_limits<size_t>::max());
            serial_through(wins.size());
        });
        int rc = ok() ? AFSK_OK : hip_fail(herr_, hwhat_);
        for (int k = 0; k < 2; k++) {
            hipError_t e = hipStreamSynchronize(copy_stream_[k]);
            if (e != hipSuccess && rc == AFSK_OK) rc = hip_fail(e, "hipStreamSynchronize");
        }
        return rc;
    }
private:
    ScratchLease lease_;
    hipStream_t copy_stream_[2] = {nullptr, nullptr};
    char* stage_[kMaxRingSlots];
    hipEvent_t event_[kMaxRingSlots];
    std::unique_ptr<std::atomic<int>[]> remaining_;   // pieces of window w still to do
    std::mutex hand_mu_;
    std::condition_variable cv_open_, cv_done_;
    size_t open_ = 0;
    std::atomic<int> failed_{0};
    hipError_t herr_ = hipSuccess;                    // the coordinator's first HIP error and the call it came from
    const char* hwhat_ = "";
};

}  // namespace
