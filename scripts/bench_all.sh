#!/bin/bash
# Every BASELINE workload on one GPU: the default C3 line with everything --full adds
# (parity check, secondary, cpu_baseline), then C2, C4, C5 and the Frankengraph with the
# parity check and secondary.  Output: $OUT/bench_<config>.json (OUT defaults to bench_out)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench_c3.json" 2> "$OUT/bench_c3.err" || exit $?
tail -1 "$OUT/bench_c3.json" | cut -c1-200
for cfg in c2 c4 c5 frank; do
  timeout -k 10 300 python -u bench.py --config $cfg --steps ${STEPS:-5} --warmup 1 --full --no-cpu-baseline \
      > "$OUT/bench_$cfg.json" 2> "$OUT/bench_$cfg.err" || { echo "$cfg failed"; tail -5 "$OUT/bench_$cfg.err"; exit 1; }
  tail -1 "$OUT/bench_$cfg.json" | cut -c1-200
done
