#!/bin/bash
# GPU tests + per-launch probe + one default bench line with its kernel trace kept
#   tools/gpu_check.sh TAG
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
TAG=${1:-chk}
OUT=${OUT:-bench_out}   # where the logs and traces of this script go
mkdir -p $OUT
fatal() { case $1 in 124|134|137|139) echo "fatal rc $1 in $2"; exit $1;; esac; }
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -4 $OUT/pytest_$TAG.log; fatal $rc pytest
if [ -n "${PROBE:-}" ]; then
  for v in 1 0; do
    A2M_GEMM_PIPE=$v timeout -k 10 150 python tools/pipe_probe.py > $OUT/probe${v}_$TAG.log 2>&1
    rc=$?; grep -E "gemm-kr|gemm 2688|conv1d B=64 Ci=256 Co=256" $OUT/probe${v}_$TAG.log; fatal $rc probe
  done
fi
A2M_BENCH_TRACE_DIR=$OUT/trace_$TAG timeout -k 10 300 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?; tail -c 3000 $OUT/bench_$TAG.json; fatal $rc bench
head -12 $OUT/trace_$TAG/step_breakdown.txt
