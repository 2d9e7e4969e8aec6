#!/bin/bash
# full bench (with cpu_baseline and every leg) + kernel-trace profile of the headline and its GPU
# legs; time-limited, chained.  Results go to $BENCH_OUT (default bench_out/ in the repository).
cd "$(dirname "$0")/../.."
R="$(pwd)"
OUT="${BENCH_OUT:-$R/bench_out}"
mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" && \
cd /tmp && export TMPDIR=/tmp && \
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- \
  python3 "$R/bench.py" --full --no-cpu --no-single-stream > "$OUT/prof_bench.json" 2> "$OUT/prof_bench.err"
