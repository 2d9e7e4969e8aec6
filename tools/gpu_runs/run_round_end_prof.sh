#!/bin/bash
# round-end evidence, part 2: the heap-sort microbenchmark, exact-mode phase counters, kernel-trace
# stats of the mapping bench (B = 128 and one stream), then one PMC pass per counter group (kernel
# trace only, no other tracing).  Results go to $BENCH_OUT (default bench_out/ in the repository).
cd "$(dirname "$0")/../.."
R="$(pwd)"
OUT="${BENCH_OUT:-$R/bench_out}"
mkdir -p "$OUT"
A="--full --no-cpu --no-single-stream --no-depth --shard-streams 0"
timeout -k 10 120 tools/bin/mb_heap > "$OUT/mb_heap.txt" 2>&1 && \
timeout -k 10 300 python -u tools/dbg_exact.py > "$OUT/dbg_exact.txt" 2>&1 && \
cd /tmp && export TMPDIR=/tmp && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python3 "$R/bench.py" $A > "$OUT/prof_bench.json" 2> "$OUT/prof_bench.err" && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof1" -o run --output-format csv -- python3 "$R/bench.py" $A --no-exact-leg --steps 30 --streams 1 --handles 1 --pipelined --no-prof > "$OUT/prof1_bench.json" 2> "$OUT/prof1_bench.err" && \
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d "$OUT/pmc_fetch" -o run --output-format csv -- python3 "$R/bench.py" $A --no-exact-leg --no-prof --steps 5 > "$OUT/pmc_fetch.json" 2> "$OUT/pmc_fetch.err" && \
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d "$OUT/pmc_write" -o run --output-format csv -- python3 "$R/bench.py" $A --no-exact-leg --no-prof --steps 5 > "$OUT/pmc_write.json" 2> "$OUT/pmc_write.err"
