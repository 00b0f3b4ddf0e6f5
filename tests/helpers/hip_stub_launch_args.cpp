// hip_stub_launch_args.cpp -- TEST INFRASTRUCTURE ONLY: the first bytes of the FIRST kernel argument of the launch made
// last, on top of hip_stub_launch.cpp (which keeps the kernel's name).  build_stub_detect_lib.sh compiles that file
// with -DhipLaunchKernel=afsk_stub_launch_inner, so the hipLaunchKernel here is the one the library's launches reach:
// it copies the bytes at launch time -- what a by-value argument struct holds then, whatever the caller does to its own
// memory afterwards -- and passes the launch on.  Never part of libafsk_amd.so.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <mutex>
#include <vector>

extern "C" hipError_t afsk_stub_launch_inner(const void*, dim3, dim3, void**, size_t, hipStream_t);

namespace {
std::mutex g_args_mu;
std::vector<unsigned char> g_args;
size_t g_want = 0;
}  // namespace

extern "C" {

// how many bytes of argument 0 the next launches copy (the test names a size its kernel's argument struct has at least)
void afsk_stub_capture_arg0(int nbytes) {
    std::lock_guard<std::mutex> lk(g_args_mu);
    g_want = nbytes > 0 ? (size_t)nbytes : 0;
    g_args.clear();
}

hipError_t hipLaunchKernel(const void* function, dim3 grid, dim3 block, void** args, size_t shared, hipStream_t stream) {
    {
        std::lock_guard<std::mutex> lk(g_args_mu);
        g_args.clear();
        if (g_want && args && args[0])
            g_args.assign(static_cast<const unsigned char*>(args[0]), static_cast<const unsigned char*>(args[0]) + g_want);
    }
    return afsk_stub_launch_inner(function, grid, block, args, shared, stream);
}

// the bytes copied at the last launch; returns how many there are
int afsk_stub_last_arg0(unsigned char* out, int cap) {
    std::lock_guard<std::mutex> lk(g_args_mu);
    const int n = (int)g_args.size();
    if (out && cap > 0) std::memcpy(out, g_args.data(), (size_t)(n < cap ? n : cap));
    return n;
}

}  // extern "C"
