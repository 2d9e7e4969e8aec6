#!/bin/bash
# round-end evidence, part 1: all GPU tests, then the full bench (cpu_baseline, stages, legs).
# Results go to $BENCH_OUT (default bench_out/ in the repository).
cd "$(dirname "$0")/../.."
OUT="${BENCH_OUT:-$(pwd)/bench_out}"
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > "$OUT/gpu_tests.log" 2>&1 && \
timeout -k 10 540 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
