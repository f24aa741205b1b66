#!/bin/bash
# GPU-box check used during development (run from the repo root):
# the -m gpu suite, then the C2 bench line, then the C3 bench line; each step
# time-limited, stopping at the first failure. Output under $OUT/.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 720 python -u -m pytest tests -m gpu -x -q -v --timeout 120 --timeout-method thread > $OUT/t1.log 2>&1 || { tail -30 $OUT/t1.log; exit 1; }
grep -E "passed|failed|PASSED.*c5|slowest" $OUT/t1.log | tail -5
timeout -k 10 240 python bench.py --full --steps 20 --stats > $OUT/b1.json 2> $OUT/b1.err || { tail -20 $OUT/b1.err; exit 1; }
timeout -k 10 200 python bench.py --full --air agg --steps 10 --no-cpu-baseline --stats > $OUT/b1agg.json 2> $OUT/b1agg.err || { tail -20 $OUT/b1agg.err; exit 1; }
timeout -k 10 120 python3 scripts/timeline.py > $OUT/timeline.txt 2>&1 || { tail -5 $OUT/timeline.txt; exit 1; }
echo ALLOK
