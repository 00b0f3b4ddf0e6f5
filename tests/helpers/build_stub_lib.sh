#!/bin/bash
# Test-only build of afsk_capi.hip's HOST code against the fake HIP runtime (hip_stub_runtime.cpp) and stub kernel
# launchers (capi_stub_launchers.hip):   build_stub_lib.sh <out> [extra hipcc flags, e.g. -fsanitize=thread]
# <out> ending in .so: the stub library the tests load.  Any other name: a stand-alone PROGRAM, the same objects
# linked statically with capi_host_driver.cpp (its own main) -- the way to run this code under a sanitizer.
# Nothing here is part of the product library.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"; ROOT="$(cd "$HERE/../.." && pwd)"
OUT=$1; shift
W=$(mktemp -d); trap 'rm -rf "$W"' EXIT
F="-O1 -g -std=c++17 -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -Wno-unused-function -fno-gpu-sanitize"
hipcc $F "$@" -c -o "$W/capi.o" "$ROOT/afskmodem_amd/csrc/afsk_capi.hip"
hipcc $F -c -o "$W/stubs.o" "$HERE/capi_stub_launchers.hip"
hipcc $F "$@" -x hip -c -o "$W/rt.o" "$HERE/hip_stub_runtime.cpp"
if [[ "$OUT" != *.so ]]; then
  hipcc $F "$@" -x hip -c -o "$W/driver.o" "$HERE/capi_host_driver.cpp"
  SAN=""; for a in "$@"; do case $a in -fsanitize=*) SAN="$SAN $a";; esac; done
  # (the driver, the entries and the fake runtime first: they define what libamdhip64 would otherwise provide)
  hipcc --offload-arch=${AFSK_ARCH:-gfx950} -fno-gpu-sanitize $SAN -o "$OUT" "$W/driver.o" "$W/capi.o" "$W/stubs.o" "$W/rt.o" -lpthread
  exit 0
fi
SAN=""; for a in "$@"; do case $a in -fsanitize=*) SAN="$a -shared-libsan";; esac; done
hipcc -fPIC --offload-arch=${AFSK_ARCH:-gfx950} -fno-gpu-sanitize $SAN -shared -Wl,-Bsymbolic -o "$OUT" "$W/capi.o" "$W/stubs.o" "$W/rt.o"
