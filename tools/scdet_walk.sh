#!/bin/bash
# k_scdet's grid on the CPU under AddressSanitizer + UBSan (tools/scdet_walk.cpp): the kernel
# file compiled for the host with the sanitizers, run here -- no GPU, no LD_PRELOAD (the
# executable carries the runtime).  Usage: tools/scdet_walk.sh
set -e
cd "$(dirname "$0")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined \
    -Xarch_host -fno-sanitize-recover=undefined scdet_walk.cpp -o scdet_walk
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 ./scdet_walk
