#!/bin/bash
# The development loop on a machine with an MI355X: the GPU test suite, then (if green) a full bench run summarised in a few lines.
# usage: [OUT_DIR=<dir>] tools/gpu_check.sh <tag> [bench args...]   (logs and the bench line under OUT_DIR, default build/check)
TAG=${1:-x}; shift
OUT=${OUT_DIR:-build/check}
mkdir -p "$OUT"
timeout -k 10 700 python -m pytest tests -m gpu -x -q > "$OUT/t_$TAG.log" 2>&1; rc=$?
tail -12 "$OUT/t_$TAG.log"; echo pytest_rc=$rc
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full "$@" > "$OUT/b_$TAG.json" 2> "$OUT/b_$TAG.err" || { tail -20 "$OUT/b_$TAG.err"; exit 1; }
python tools/bench_summary.py "$OUT/b_$TAG.json"
