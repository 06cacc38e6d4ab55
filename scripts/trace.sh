#!/bin/bash
# rocprofv3 kernel trace (+ --stats) of the C2 bench (--full: the roofline legs are cross-checked against the trace);
# raw CSVs in a scratch directory, summaries to $FD_OUT/<tag>_* (default: trace_out/ in the repository):
# per-step window anatomy, per-instance GEMM table, roofline cross-check against the bench line, kernel stats.
# Usage: scripts/trace.sh <tag> [extra bench.py args]
cd "$(dirname "$0")/.."
R=$(pwd)
TAG=${1:-trace}; shift
export TMPDIR=/tmp
D=/tmp/fdprof/bench
O=${FD_OUT:-$R/trace_out}
rm -rf $D; mkdir -p $D $O
(cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $D -o run \
   -- python3 $R/bench.py --full --no-cpu-baseline --no-c3 --no-pipeline --steps 20 --warmup 3 "$@" > $O/${TAG}_prof_bench.log 2>&1)
rc=$?; echo "rocprof rc=$rc"; tail -c 300 $O/${TAG}_prof_bench.log; [ $rc -eq 0 ] || exit $rc
T=$(find $D -name "*kernel_trace.csv" | head -1)
python3 scripts/prof_window.py $T 3 > $O/${TAG}_step_window.txt || exit 1
python3 scripts/roofline_check.py $T $O/${TAG}_prof_bench.log 3 > $O/${TAG}_roofline_check.json || exit 1
python3 scripts/prof_gemm_breakdown.py $T 3 > $O/${TAG}_gemm_instances.txt 2>&1 || true
python3 scripts/prof_positions.py $T 3 > $O/${TAG}_positions.txt 2>&1 || true
cp $(find $D -name "*kernel_stats.csv" | head -1) $O/${TAG}_kernel_stats.csv
gzip -c $T > $O/${TAG}_kernel_trace.csv.gz  # the raw trace, for off-box analysis (scripts/prof_*.py read .gz)
head -20 $O/${TAG}_step_window.txt; cat $O/${TAG}_roofline_check.json
