#!/bin/bash
# rocprofv3 kernel trace of recommend() alone (tests/manual/recommend_timing.py --only-b), in a run
# of its own, and its per-kernel summary (profiles/recommend_trace_summary.py).  Run on the GPU box
# from the repository root: profiles/recommend_prof.sh [output directory (default: a fresh temporary one)]
set -o pipefail
OUT=${1:-$(mktemp -d)}
echo "output directory: $OUT"
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/recommend_prof -- \
  python tests/manual/recommend_timing.py --only-b --repeats 3 > $OUT/recommend_prof.txt 2>&1 || { tail -20 $OUT/recommend_prof.txt; exit 1; }
F=$(find $OUT/recommend_prof -name "*kernel_trace.csv" | head -1)
python profiles/recommend_trace_summary.py "$F" | tee $OUT/recommend_trace_summary.txt
