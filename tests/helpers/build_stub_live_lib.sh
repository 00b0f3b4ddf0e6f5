#!/bin/bash
# Test-only build of the HOST code of afsk_capi.hip, afsk_gate.hip (the gate, the split plan, the live receivers and
# the rate detector) and afsk_synth.hip (the live transmitter) against the fake HIP runtime (hip_stub_runtime.cpp +
# hip_stub_launch.cpp):   build_stub_live_lib.sh <out.so>
# afsk_gate.hip and afsk_synth.hip are compiled host-only: their kernels register by name and "launch" without running,
# so the live entries run start to finish on the CPU and a test sees which kernels an entry launched, in what order and
# with what first argument.  The demod launchers of afsk_demod*.hip are stubs that note their call in the launch log as
# "demod".  Every stub test of these units loads this one library (tests/stub_lib.py).  Nothing here is part of the
# product library.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$(cd "$HERE/../.." && pwd)"
OUT=$1; shift
W=$(mktemp -d); trap 'rm -rf "$W"' EXIT
cat > "$W/stubs.hip" <<S
#include "$ROOT/afskmodem_amd/csrc/afsk_kernels.h"
extern "C" void afsk_stub_log_note(const char*);
namespace afsk {
hipError_t launch_demod(const DemodArgs&, hipStream_t) { afsk_stub_log_note("demod"); return hipSuccess; }
hipError_t launch_demod_uniform(const DemodArgs&, hipStream_t) { afsk_stub_log_note("demod"); return hipSuccess; }
}
S
F="-O1 -g -std=c++17 -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -Wno-unused-function -fno-gpu-sanitize"
hipcc $F -c -o "$W/capi.o" "$ROOT/afskmodem_amd/csrc/afsk_capi.hip" &
hipcc $F --offload-host-only -c -o "$W/gate.o" "$ROOT/afskmodem_amd/csrc/afsk_gate.hip" &
hipcc $F --offload-host-only -c -o "$W/synth.o" "$ROOT/afskmodem_amd/csrc/afsk_synth.hip" &
hipcc $F -c -o "$W/stubs.o" "$W/stubs.hip" &
hipcc $F -x hip -c -o "$W/rt.o" "$HERE/hip_stub_runtime.cpp" &
hipcc $F -x hip -c -o "$W/launch.o" "$HERE/hip_stub_launch.cpp" &
for j in $(jobs -p); do wait "$j"; done
# the host-only objects refer to the device binaries they were not given: point those symbols at a dummy
DEF=""; for s in $(nm -u "$W/gate.o" "$W/synth.o" | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u); do DEF="$DEF -Wl,--defsym=$s=afsk_stub_fatbin"; done
hipcc -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -fno-gpu-sanitize -shared -Wl,-Bsymbolic $DEF -o "$OUT" \
  "$W/capi.o" "$W/gate.o" "$W/synth.o" "$W/stubs.o" "$W/rt.o" "$W/launch.o"
