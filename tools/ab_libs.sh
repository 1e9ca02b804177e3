#!/bin/bash
# A/B of libdts builds on the cfg2 bench: tools/ab_libs.sh <lib-suffix>... ("" or base = lib/libdts.so)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
L=distributed-transcoding-server_amd/lib
OUT=${AB_OUT:-ab_out}   # where the bench logs go
mkdir -p "$OUT"
for v in "$@"; do
  [ "$v" = base ] && v=""
  lib=$L/libdts${v:+_$v}.so
  for wl in ${AB_WORKLOADS:-cfg2}; do
    log=$OUT/ab_${v:-base}_$wl.log
    DTS_LIB=$PWD/$lib timeout -k 10 200 python -u bench.py --steps 20 --warmup 3 --full --no-cpu --workload $wl > $log 2>&1
    rc=$?
    echo "== ${v:-base} $wl rc=$rc $(grep -o '"value": [0-9.]*' $log) $(grep -o '"frac": [0-9.]*' $log) $(grep -o '"verified_vs_oracle": [a-z]*' $log)"
    [ $rc -ge 124 ] && exit $rc
  done
done
exit 0
