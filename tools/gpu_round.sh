#!/bin/bash
# One GPU session: parity tests, bench, rocprofv3 kernel stats.  Each GPU step has its own limit.
#   [OUT=dir] bash tools/gpu_round.sh [all|test|bench|prof|pmc]    (results under OUT, default bench_out/)
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT" || exit 1
OUT=${OUT:-$ROOT/bench_out}
mkdir -p "$OUT"
OUT=$(cd "$OUT" && pwd)
export TMPDIR=/tmp
step=${1:-all}
if [[ $step == all || $step == test ]]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { echo "pytest failed"; tail -40 "$OUT/pytest_gpu.log"; exit 1; }
  tail -3 "$OUT/pytest_gpu.log"
fi
if [[ $step == all || $step == bench ]]; then
  # the long line: every leg beside the headline is behind --full
  timeout -k 10 400 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo "bench failed"; tail -30 "$OUT/bench.err"; exit 1; }
  cat "$OUT/bench.json"
fi
if [[ $step == all || $step == prof ]]; then
  cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 "$ROOT/bench.py" --full --steps 10 --no-cpu --latency-runs 0 > "$OUT/prof_bench.json" 2> "$OUT/prof.err" || { echo "rocprof failed"; tail -30 "$OUT/prof.err"; exit 1; }
  cd "$ROOT"; find "$OUT/prof" -name "*kernel_stats.csv" | head -3
fi
if [[ $step == all || $step == pmc ]]; then
  # one counter group per pass (gfx950 slot limits: 8 SQ, 4 TCC; FETCH_SIZE uses 3, WRITE_SIZE 2)
  cd /tmp
  i=0
  for grp in "SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU" \
             "SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_LDS SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_INT64 SQ_WAIT_INST_LDS" \
             "FETCH_SIZE" "WRITE_SIZE"; do
    i=$((i+1))
    timeout -s KILL 120 rocprofv3 --kernel-trace --output-format csv --pmc $grp -d "$OUT/pmc$i" -o run -- python3 "$ROOT/bench.py" --full --steps 3 --warmup 1 --no-cpu --latency-runs 0 --no-extras > "$OUT/pmc$i.json" 2> "$OUT/pmc$i.err" || { echo "pmc pass $i failed"; tail -20 "$OUT/pmc$i.err"; exit 1; }
  done
  cd "$ROOT"; find "$OUT" -name "*counter_collection.csv" | head
fi
