#!/bin/bash
# Test-only build of the HOST code of afsk_capi.hip and afsk_gate.hip (with it the rate detector, afsk_detect.hip)
# against the fake HIP runtime:   build_stub_detect_lib.sh <out.so>
# As build_stub_live_lib.sh, with a copy of the launch's first argument (hip_stub_launch_args.cpp:
# afsk_stub_capture_arg0 / afsk_stub_last_arg0), so a test sees what an entry passed to its kernel BY VALUE.  Nothing
# here is part of the product library.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$(cd "$HERE/../.." && pwd)"
OUT=$1; shift
W=$(mktemp -d); trap 'rm -rf "$W"' EXIT
cat > "$W/stubs.hip" <<S
#include "$ROOT/afskmodem_amd/csrc/afsk_kernels.h"
namespace afsk {
hipError_t launch_demod(const DemodArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_demod_uniform(const DemodArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_modulate(ModulateArgs, int32_t, hipStream_t) { return hipSuccess; }
hipError_t launch_noise(NoiseArgs, int32_t, hipStream_t) { return hipSuccess; }
}
S
F="-O1 -g -std=c++17 -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -Wno-unused-function -fno-gpu-sanitize"
hipcc $F -c -o "$W/capi.o" "$ROOT/afskmodem_amd/csrc/afsk_capi.hip" &
hipcc $F --offload-host-only -c -o "$W/gate.o" "$ROOT/afskmodem_amd/csrc/afsk_gate.hip" &
wait
hipcc $F -c -o "$W/stubs.o" "$W/stubs.hip"
hipcc $F -x hip -c -o "$W/rt.o" "$HERE/hip_stub_runtime.cpp"
hipcc $F -x hip -DhipLaunchKernel=afsk_stub_launch_inner -c -o "$W/launch.o" "$HERE/hip_stub_launch.cpp"
hipcc $F -x hip -c -o "$W/args.o" "$HERE/hip_stub_launch_args.cpp"
# the host-only object refers to the device binary it was not given: point that symbol at a dummy
DEF=""; for s in $(nm -u "$W/gate.o" | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u); do DEF="$DEF -Wl,--defsym=$s=afsk_stub_fatbin"; done
hipcc -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -fno-gpu-sanitize -shared -Wl,-Bsymbolic $DEF -o "$OUT" \
  "$W/capi.o" "$W/gate.o" "$W/stubs.o" "$W/rt.o" "$W/launch.o" "$W/args.o"
