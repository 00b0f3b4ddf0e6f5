// hip_stub_launch.cpp -- TEST INFRASTRUCTURE ONLY: what hip_stub_runtime.cpp lacks to run the HOST code of a translation
// unit that holds kernels (afsk_gate.hip: the live receivers) on the CPU.  Kernels register by name and "launch" without
// running: a launch records the kernel's name and its grid, so a test sees which kernel an entry chose.  hipMemsetAsync
// fills host memory.  Linked (with -Bsymbolic) into a test-only build of the library (build_stub_live_lib.sh); never
// part of libafsk_amd.so.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <map>
#include <mutex>
#include <string>

namespace {
std::mutex g_mu;
std::map<const void*, std::string>& names() {
    static std::map<const void*, std::string> m;
    return m;
}
std::string g_last;
unsigned g_last_grid = 0, g_launches = 0;
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
hipError_t hipLaunchKernel(const void* function, dim3 grid, dim3, void**, size_t, hipStream_t) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = names().find(function);
    g_last = it == names().end() ? "?" : it->second;
    g_last_grid = grid.x;
    g_launches++;
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

}  // extern "C"
