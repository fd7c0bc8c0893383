#!/bin/bash
# Banded long rows against a parent build: default run A/B, band-size sweep, one front vs the strided
# grid, the other workloads, kernel traces.  Run on the GPU box.  usage: tools/band_sweep.sh <output directory> <parent libmyrrix_als.so>
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m $1)
PARENT=$(realpath $2)
mkdir -p $OUT
cd $ROOT
MB=1048576
run() {  # tag, then env assignments, then -- bench args
  local tag=$1; shift
  local envs=()
  while [ "$1" != "--" ]; do envs+=("$1"); shift; done
  shift
  env "${envs[@]}" timeout -k 10 300 python bench.py "$@" > $OUT/$tag.json 2> $OUT/$tag.err
  local rc=$?
  if [ $rc -ne 0 ]; then echo "STOP: $tag rc=$rc"; tail -5 $OUT/$tag.err; exit $rc; fi
  echo "done $tag"
}
# 1. A/B on the default run, alternating
for i in 1 2 3 4; do
  run ab_parent_$i MALS_LIB=$PARENT --
  run ab_new_$i X=1 --
done
# 2. sweep of the band size (front), off, and strided
for i in 1 2; do
  run sw_off_$i MALS_BAND_BYTES=0 --
  for mb in 16 32 48 64 96 128; do
    run sw_front_${mb}_$i MALS_BAND_BYTES=$((mb * MB)) --
  done
  for mb in 32 64; do
    run sw_strided_${mb}_$i MALS_BAND_BYTES=$((mb * MB)) MALS_BAND_FRONT=0 --
  done
done
# 3. the other workloads, parent against new
for i in 1 2 3; do
  run unpl_parent_$i MALS_LIB=$PARENT -- --planted 0
  run unpl_new_$i X=1 -- --planted 0
  for wl in c2 c3 c4rank; do
    run ${wl}_parent_$i MALS_LIB=$PARENT -- --workload $wl
    run ${wl}_new_$i X=1 -- --workload $wl
  done
done
# 4. kernel traces of the default run
export TMPDIR=/tmp
for v in parent new; do
  if [ $v = parent ]; then L="MALS_LIB=$PARENT"; else L="X=1"; fi
  ( cd /tmp && env $L timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT/trace_$v -o bench -- python $ROOT/bench.py > $OUT/traced_$v.json 2> $OUT/traced_$v.err )
  rc=$?
  if [ $rc -ne 0 ]; then echo "STOP: trace $v rc=$rc"; tail -5 $OUT/traced_$v.err; exit $rc; fi
  DB=$(find $OUT/trace_$v -name "*.db" | head -1)
  python tools/rocprof_summary.py $DB > $OUT/kernel_stats_$v.txt 2>&1 || true
  rm -rf $OUT/trace_$v
  head -8 $OUT/kernel_stats_$v.txt
done
python tools/bench_summary.py $OUT
