#!/bin/bash
# AddressSanitizer + UBSan run of the owning device-buffer type (raleigh_amd/csrc/device_mem.h) on the host: the driver
# stands in for the allocation point with malloc / free (CPU build: GPU sanitizers are not available on this pool).
# usage: tools/device_mem_sanitize.sh   (here or on any box; needs only the ROCm clang)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
O=${TMPDIR:-/tmp}/rlh_device_mem_asan; mkdir -p $O
${HIPCLANG:-/opt/rocm/lib/llvm/bin/clang++} -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  -fno-omit-frame-pointer -I $R/raleigh_amd/csrc $R/tools/device_mem_main.cpp -o $O/device_mem_asan
$O/device_mem_asan
