#!/bin/bash
# Round-6 profiles (GPU box): PMC traffic + SQ passes for C2 and C3 (scripts/profile_round.sh),
# then the kernel trace (--stats) of the judged bench command itself.
set -o pipefail
OUT=${OUT:-bench_out}
export TMPDIR=/tmp
mkdir -p $OUT
bash scripts/profile_round.sh r06_c2 > $OUT/prof_c2.out 2>&1 || { tail -5 $OUT/prof_c2.out; exit 1; }
bash scripts/profile_round.sh r06_c3 --air agg > $OUT/prof_c3.out 2>&1 || { tail -5 $OUT/prof_c3.out; exit 1; }
if [ "${1:-}" = "judged" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_judged -o run -- \
    python3 bench.py --full --steps 20 --warmup 5 > $OUT/prof_judged.json 2> $OUT/prof_judged.err || { tail -5 $OUT/prof_judged.err; exit 1; }
fi
echo PROFOK
