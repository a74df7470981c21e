#!/bin/bash
# rocprofv3 kernel trace (no counters) of rank_catalogue()'s launches and of rfm_pair_topk's at
# k = 64 (the floor), tests/manual/rank_catalogue_timing.py --device-only, in a run of its own, and
# its per-kernel summary (profiles/rank_catalogue_trace_summary.py).  Run on the GPU box from the
# repository root: profiles/rank_catalogue_prof.sh [output directory (default: a fresh temporary one)]
set -o pipefail
OUT=${1:-$(mktemp -d)}
echo "output directory: $OUT"
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rank_catalogue_prof -- \
  python tests/manual/rank_catalogue_timing.py --device-only $OUT/rank_catalogue_plan.json > $OUT/rank_catalogue_prof.txt 2>&1 || { tail -20 $OUT/rank_catalogue_prof.txt; exit 1; }
F=$(find $OUT/rank_catalogue_prof -name "*kernel_trace.csv" | head -1)
python profiles/rank_catalogue_trace_summary.py "$F" $OUT/rank_catalogue_plan.json | tee $OUT/rank_catalogue_trace_summary.txt
