#!/bin/bash
# rocprofv3 kernel trace of rank_items()'s launches and of rfm_pair_scores' (the floor of one pass
# over the product), tests/manual/rank_items_timing.py --device-only, in a run of its own, and its
# per-kernel summary (profiles/rank_items_trace_summary.py).  Run on the GPU box from the
# repository root: profiles/rank_items_prof.sh [output directory (default: a fresh temporary one)]
set -o pipefail
OUT=${1:-$(mktemp -d)}
echo "output directory: $OUT"
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/rank_items_prof -- \
  python tests/manual/rank_items_timing.py --device-only > $OUT/rank_items_prof.txt 2>&1 || { tail -20 $OUT/rank_items_prof.txt; exit 1; }
F=$(find $OUT/rank_items_prof -name "*kernel_trace.csv" | head -1)
python profiles/rank_items_trace_summary.py "$F" | tee $OUT/rank_items_trace_summary.txt
