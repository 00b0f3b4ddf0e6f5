// afsk_host_pool.h -- the CPU side of the host entries' data path: where the device's NUMA node is, how many CPUs
// this process may use, the persistent fork-safe I/O pool and the parallel memcpy built on it.  Host code only,
// included by afsk_capi.hip alone (everything here has internal linkage).
#pragma once

#include <hip/hip_runtime.h>

#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace {

// ---- NUMA: keep the host side of the PCIe traffic on the socket the GPU hangs off ---------------------------
// The GPU boxes are two-socket hosts (2 x 64 cores, 4 GPUs per socket).  A staging buffer pinned on the other
// socket is read by the GPU across the inter-socket link (43 instead of 57 GB/s measured), and pool threads on
// the other socket copy page-cache pages into it at half the rate (read 100 ms instead of 55 ms of CPU per 393 MB).
// So: the pinned staging buffers are allocated while the calling thread is (temporarily) confined to the CPUs of
// the device's NUMA node, and the I/O pool's threads stay on those CPUs.  AFSK_NUMA_BIND=0 turns both off;
// anything that cannot be found out (no such attribute, no sysfs) means "no binding", never an error.
bool device_node_cpus(cpu_set_t* out) {
    static const bool enabled = [] { const char* e = std::getenv("AFSK_NUMA_BIND"); return !e || std::atoi(e) != 0; }();
    if (!enabled) return false;
    int dev = 0, node = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    // one answer per device and process (two sysfs reads otherwise, on every ingest call); a process that
    // drives GPUs on both sockets gets each device's own node
    constexpr int kMaxCachedDevices = 64;
    static std::mutex cache_mu;
    static bool known[kMaxCachedDevices], known_ok[kMaxCachedDevices];
    static cpu_set_t known_cpus[kMaxCachedDevices];
    std::lock_guard<std::mutex> cache_lock(cache_mu);
    const bool cacheable = dev >= 0 && dev < kMaxCachedDevices;
    if (cacheable && known[dev]) { if (known_ok[dev]) *out = known_cpus[dev]; return known_ok[dev]; }
    if (cacheable) { known[dev] = true; known_ok[dev] = false; }
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, dev) != hipSuccess || node < 0) {
        (void)hipGetLastError();
        node = -1;
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, dev) != hipSuccess) { (void)hipGetLastError(); return false; }
        for (char* c = bus; *c; c++) *c = (char)std::tolower((unsigned char)*c);
        const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
        if (FILE* f = std::fopen(path.c_str(), "r")) {
            if (std::fscanf(f, "%d", &node) != 1) node = -1;
            std::fclose(f);
        }
    }
    if (node < 0) return false;
    char path[96];
    std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    cpu_set_t allowed, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) { std::fclose(f); return false; }
    int a = 0, b = 0;
    for (;;) {                                             // "0-63,128-191"
        if (std::fscanf(f, "%d", &a) != 1) break;
        b = a;
        int c = std::fgetc(f);
        if (c == '-') { if (std::fscanf(f, "%d", &b) != 1) break; c = std::fgetc(f); }
        for (int k = a; k <= b && k < CPU_SETSIZE; k++)
            if (CPU_ISSET(k, &allowed)) CPU_SET(k, &want);
        if (c != ',') break;
    }
    std::fclose(f);
    if (CPU_COUNT(&want) == 0) return false;
    *out = want;
    if (cacheable) { known_cpus[dev] = want; known_ok[dev] = true; }
    return true;
}

// confines the calling thread to the device's NUMA node for its lifetime (allocations made meanwhile are
// first-touched there), then restores the thread's affinity
class NodeBinder {
public:
    NodeBinder() {
        cpu_set_t want;
        if (!device_node_cpus(&want)) return;
        if (pthread_getaffinity_np(pthread_self(), sizeof old_, &old_) != 0) return;
        bound_ = pthread_setaffinity_np(pthread_self(), sizeof want, &want) == 0;
    }
    ~NodeBinder() {
        if (bound_) (void)pthread_setaffinity_np(pthread_self(), sizeof old_, &old_);
    }
private:
    cpu_set_t old_;
    bool bound_ = false;
};

// CPUs this process may really use: the cgroup CPU quota (v2 cpu.max, v1 cfs_quota_us / cfs_period_us) where one
// is set -- hardware_concurrency() reports every core of the host (256 on the GPU boxes, whose containers get
// the time of 16), and a pool sized for cores the scheduler will not grant is throttled for whole 100 ms
// periods (the 60 - 180 ms outliers of the r3 ingest) -- else the affinity mask / core count.
unsigned usable_cpus() {
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) hw = std::min(hw, (unsigned)std::max(1, CPU_COUNT(&set)));
    long long quota = -1, period = 100000;
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0) quota = std::atoll(q);
        std::fclose(f);
    } else if (FILE* g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        if (std::fscanf(g, "%lld", &quota) != 1) quota = -1;
        std::fclose(g);
        if (FILE* h = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (std::fscanf(h, "%lld", &period) != 1) period = 100000;
            std::fclose(h);
        }
    }
    if (quota > 0 && period > 0) hw = std::min<unsigned>(hw, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
    // one process per GPU: the rank processes of a node (LOCAL_WORLD_SIZE, set by torchrun and by bench.py's
    // launcher) share these CPUs -- eight ranks with a quota's worth of threads each are throttled together
    if (const char* e = std::getenv("LOCAL_WORLD_SIZE")) {
        const int lw = std::atoi(e);
        if (lw > 1) hw = std::max(1u, hw / (unsigned)lw);
    }
    return hw;
}

unsigned io_threads() {
    static const unsigned v = [] {
        const char* e = std::getenv("AFSK_IO_THREADS");
        return e ? (unsigned)std::max(1, std::atoi(e)) : std::min(32u, usable_cpus());
    }();
    return v;
}

// A small persistent pool for the file-ingest entries: spawning 15 threads per staging window cost
// more than filling the window.  run(n, width, body) executes body(i) for i in [0, n) on up to
// `width` threads (the caller is one of them) and returns when all are done; one job at a time.
class IoPool {
public:
    // from the next job on the pool's threads stay on these CPUs (the device's NUMA node).  Called by the
    // entries that talk to the device anyway -- never by the host-only ones (afsk_wav_probe, afsk_file_sizes
    // make no HIP call, also not to find out where the device lives).
    // A later call with another mask (the same process ingesting for a GPU on the other socket) moves the
    // threads: every worker re-applies the affinity when the mask's version differs from the one it applied.
    void confine_to(const cpu_set_t& cpus) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!confined_ || !CPU_EQUAL(&cpus_, &cpus)) { cpus_ = cpus; confined_ = true; cpus_ver_++; }
    }
    ~IoPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    template <class F>
    void run(size_t n, unsigned width, F&& body) {
        if (n == 0) return;
        if (width <= 1 || n == 1) {
            for (size_t i = 0; i < n; i++) body(i);
            return;
        }
        std::lock_guard<std::mutex> job_lock(job_mu_);        // one job at a time
        grow(std::min<size_t>(width - 1, n - 1));
        std::function<void(size_t)> fn = std::ref(body);
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn; n_ = n; next_.store(0); busy_ = th_.size(); gen_++;
        }
        cv_.notify_all();
        drain(fn, n);
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return busy_ == 0; });
        fn_ = nullptr;
    }
    // body(i) for i in [0, n) on POOL threads only (at least `width` of them exist afterwards, thread creation
    // permitting) while the caller runs main_fn(have_workers) -- a coordinator that consumes what the workers
    // produce; returns when both are done.  When no pool thread could be started main_fn is told so
    // (have_workers == false) and has to run the tasks itself: run_split never does.  One job at a time:
    // job_mu_ is held for the whole call, so a concurrent run() / run_split() of another thread waits.
    template <class F, class M>
    void run_split(size_t n, unsigned width, F&& body, M&& main_fn) {
        std::lock_guard<std::mutex> job_lock(job_mu_);
        grow(std::max<size_t>(1, std::min<size_t>(width, n)));
        std::function<void(size_t)> fn = std::ref(body);
        const bool have_workers = !th_.empty() && n > 0;
        if (have_workers) {
            {
                std::lock_guard<std::mutex> lk(mu_);
                fn_ = &fn; n_ = n; next_.store(0); busy_ = th_.size(); gen_++;
            }
            cv_.notify_all();
        }
        main_fn(have_workers);
        if (have_workers) {
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [&] { return busy_ == 0; });
            fn_ = nullptr;
        }
    }
private:
    void drain(const std::function<void(size_t)>& fn, size_t n) {
        for (;;) {
            const size_t i = next_.fetch_add(1, std::memory_order_relaxed);
            if (i >= n) return;
            fn(i);
        }
    }
    void grow(size_t want) {
        uint64_t gen_now;
        {
            std::lock_guard<std::mutex> lk(mu_);
            gen_now = gen_;                                     // a new worker starts with the NEXT job
        }
        while (th_.size() < want) {
            try {
                th_.emplace_back([this, gen_now] { worker(gen_now); });
            } catch (...) {
                break;                                          // fewer helpers: the caller drains the rest
            }
        }
    }
    void worker(uint64_t seen) {
        uint64_t applied_ver = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return quit_ || gen_ != seen; });
            if (quit_) return;
            seen = gen_;
            if (confined_ && applied_ver != cpus_ver_) {
                (void)pthread_setaffinity_np(pthread_self(), sizeof cpus_, &cpus_);
                applied_ver = cpus_ver_;
            }
            const std::function<void(size_t)>* fn = fn_;
            const size_t n = n_;
            lk.unlock();
            if (fn) drain(*fn, n);
            lk.lock();
            if (--busy_ == 0) done_cv_.notify_all();
        }
    }
    cpu_set_t cpus_;
    uint64_t cpus_ver_ = 0;
    bool confined_ = false;
    std::mutex mu_, job_mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> th_;
    const std::function<void(size_t)>* fn_ = nullptr;
    size_t n_ = 0, busy_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t gen_ = 0;
    bool quit_ = false;
};
// Never destroyed (no join of parked threads at process exit) and FORK-SAFE: after fork() the child
// has the parent's pool object but none of its threads -- run() would wait for workers that do not
// exist -- so a pthread_atfork child handler abandons the inherited pool (leaked on purpose: its
// std::thread objects are joinable and its mutexes may be held by threads that are gone) and the
// child's first call builds a fresh one.
std::atomic<IoPool*> g_io_pool{nullptr};
std::mutex g_io_pool_mu;
void io_pool_after_fork_in_child() {
    g_io_pool.store(nullptr, std::memory_order_relaxed);
    new (&g_io_pool_mu) std::mutex();            // the parent may have held it at fork time
}
IoPool& io_pool() {
    IoPool* p = g_io_pool.load(std::memory_order_acquire);
    if (p) return *p;
    std::lock_guard<std::mutex> lk(g_io_pool_mu);
    p = g_io_pool.load(std::memory_order_relaxed);
    if (!p) {
        static const int registered = pthread_atfork(nullptr, nullptr, io_pool_after_fork_in_child);
        (void)registered;
        p = new IoPool();
        g_io_pool.store(p, std::memory_order_release);
    }
    return *p;
}
// the pool's threads belong on the current device's socket (one process per GPU)
void confine_pool_to_device_node() {
    cpu_set_t cpus;
    if (device_node_cpus(&cpus)) io_pool().confine_to(cpus);
}

struct CopyJob { char* dst; const char* src; size_t bytes; };

// memcpy a list of pieces, split over the I/O pool's threads when it is worth it (one core moves ~30 GB/s into
// pinned memory from a hot source, a few GB/s from cold pages; the PCIe link takes ~56 GB/s: tools/h2d_probe).
// (r4: the persistent pool instead of std::threads spawned per staging window -- ~100 thread creations per call of
// the gather entry at 4096 streams.)
void parallel_copy(const std::vector<CopyJob>& jobs, size_t total) {
    static const unsigned max_threads = [] {
        const char* e = std::getenv("AFSK_COPY_THREADS");
        return e ? (unsigned)std::max(1, std::atoi(e)) : std::min(16u, std::max(1u, usable_cpus()));
    }();
    unsigned nt = total >= ((size_t)4 << 20) ? max_threads : 1u;
    if (nt <= 1) {
        for (const CopyJob& j : jobs) std::memcpy(j.dst, j.src, j.bytes);
        return;
    }
    // split the byte range into nt contiguous shares
    const size_t share = (total + nt - 1) / nt;
    std::vector<std::vector<CopyJob>> parts;
    size_t ji = 0, joff = 0;                       // cursor: job index, byte offset inside it
    while (ji < jobs.size()) {
        std::vector<CopyJob> mine;
        size_t left = share;
        while (left > 0 && ji < jobs.size()) {
            const size_t take = std::min(left, jobs[ji].bytes - joff);
            if (take > 0) mine.push_back({jobs[ji].dst + joff, jobs[ji].src + joff, take});
            left -= take; joff += take;
            if (joff == jobs[ji].bytes) { ji++; joff = 0; }
        }
        parts.push_back(std::move(mine));
    }
    io_pool().run(parts.size(), (unsigned)parts.size(), [&](size_t k) {
        for (const CopyJob& j : parts[k]) std::memcpy(j.dst, j.src, j.bytes);
    });
}

}  // namespace
