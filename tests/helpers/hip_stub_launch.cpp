// hip_stub_launch.cpp -- TEST INFRASTRUCTURE ONLY: what hip_stub_runtime.cpp lacks to run the HOST code of translation
// units that hold kernels (afsk_gate.hip: the live receivers, afsk_synth.hip: the live transmitter) on the CPU.  Kernels
// register by name and "launch" without running.  A launch records the kernel's name, its grid and the launch count
// (afsk_stub_last_kernel), appends the name to a log of ALL launches in order (afsk_stub_kernel_log), and, once a test
// has set a size with afsk_stub_capture_arg0, copies that many bytes of the FIRST kernel argument (afsk_stub_last_arg0):
// what a by-value argument struct holds at launch time, whatever the caller does to its own memory afterwards.
// hipMemsetAsync fills host memory.  Linked (with -Bsymbolic) into a test-only build of the library
// (build_stub_live_lib.sh); never part of libafsk_amd.so.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {
std::mutex g_mu;
std::map<const void*, std::string>& names() {
    static std::map<const void*, std::string> m;
    return m;
}
std::string g_last, g_log;
unsigned g_last_grid = 0, g_launches = 0;
std::vector<unsigned char> g_args;
size_t g_want = 0;
struct Config {
    dim3 grid, block;
    size_t shared;
    hipStream_t stream;
};
thread_local Config t_cfg;
}  // namespace

extern "C" {

char afsk_stub_fatbin[8] = {0};       // what a host-only compile's __hip_fatbin_<hash> is pointed at (never read)

void** __hipRegisterFatBinary(const void*) {
    static void* handle = nullptr;
    return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_function, char*, const char* device_name, unsigned int, void*, void*,
                           void*, void*, int*) {
    std::lock_guard<std::mutex> lk(g_mu);
    names()[host_function] = device_name;
}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shared, hipStream_t stream) {
    t_cfg = Config{grid, block, shared, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shared, hipStream_t* stream) {
    *grid = t_cfg.grid;
    *block = t_cfg.block;
    *shared = t_cfg.shared;
    *stream = t_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* function, dim3 grid, dim3, void** args, size_t, hipStream_t) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = names().find(function);
    g_last = it == names().end() ? "?" : it->second;
    g_last_grid = grid.x;
    g_launches++;
    g_log += g_last;
    g_log += '\n';
    g_args.clear();
    if (g_want && args && args[0])
        g_args.assign(static_cast<const unsigned char*>(args[0]), static_cast<const unsigned char*>(args[0]) + g_want);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    std::memset(d, v, n);
    return hipSuccess;
}

// the mangled name of the kernel launched last (empty: none yet); returns the launches so far
int afsk_stub_last_kernel(char* out, int cap, unsigned* out_grid_x) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (out && cap > 0) {
        std::strncpy(out, g_last.c_str(), (size_t)cap - 1);
        out[cap - 1] = 0;
    }
    if (out_grid_x) *out_grid_x = g_last_grid;
    return (int)g_launches;
}

// a launcher that is itself a stub (build_stub_live_lib.sh's demod launchers) notes its call in the log
void afsk_stub_log_note(const char* what) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_log += what;
    g_log += '\n';
}

// the mangled names launched since the last clear, one per line; returns the bytes the whole log needs
int afsk_stub_kernel_log(char* out, int cap, int clear) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (out && cap > 0) {
        std::strncpy(out, g_log.c_str(), (size_t)cap - 1);
        out[cap - 1] = 0;
    }
    const int need = (int)g_log.size() + 1;
    if (clear) g_log.clear();
    return need;
}

// how many bytes of argument 0 the next launches copy (the test names a size its kernel's argument struct has at
// least); 0, the default: no copy
void afsk_stub_capture_arg0(int nbytes) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_want = nbytes > 0 ? (size_t)nbytes : 0;
    g_args.clear();
}

// the bytes copied at the last launch; returns how many there are
int afsk_stub_last_arg0(unsigned char* out, int cap) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int n = (int)g_args.size();
    if (out && cap > 0) std::memcpy(out, g_args.data(), (size_t)(n < cap ? n : cap));
    return n;
}

}  // extern "C"
