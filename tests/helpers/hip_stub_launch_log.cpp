// hip_stub_launch_log.cpp -- TEST INFRASTRUCTURE ONLY: the names of ALL kernels launched, in order, on top of
// hip_stub_launch.cpp (which keeps the last one).  build_stub_ragged_lib.sh compiles that file with
// -DhipLaunchKernel=afsk_stub_launch_inner, so the hipLaunchKernel here is the one the library's launches reach: it
// passes the launch on and appends the name it recorded.  Never part of libafsk_amd.so.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>
#include <string>

extern "C" {
hipError_t afsk_stub_launch_inner(const void*, dim3, dim3, void**, size_t, hipStream_t);
int afsk_stub_last_kernel(char* out, int cap, unsigned* out_grid_x);
}

namespace {
std::mutex g_log_mu;
std::string g_log;
}  // namespace

extern "C" {

hipError_t hipLaunchKernel(const void* function, dim3 grid, dim3 block, void** args, size_t shared, hipStream_t stream) {
    const hipError_t e = afsk_stub_launch_inner(function, grid, block, args, shared, stream);
    char name[512];
    afsk_stub_last_kernel(name, (int)sizeof name, nullptr);
    std::lock_guard<std::mutex> lk(g_log_mu);
    g_log += name;
    g_log += '\n';
    return e;
}

// a launcher that is itself a stub (build_stub_ragged_lib.sh's demod launchers) notes its call in the log
void afsk_stub_log_note(const char* what) {
    std::lock_guard<std::mutex> lk(g_log_mu);
    g_log += what;
    g_log += '\n';
}

// the mangled names launched since the last clear, one per line; returns the bytes the whole log needs
int afsk_stub_kernel_log(char* out, int cap, int clear) {
    std::lock_guard<std::mutex> lk(g_log_mu);
    if (out && cap > 0) {
        std::strncpy(out, g_log.c_str(), (size_t)cap - 1);
        out[cap - 1] = 0;
    }
    const int need = (int)g_log.size() + 1;
    if (clear) g_log.clear();
    return need;
}

}  // extern "C"
