#!/bin/bash
# rocprofv3 traces (no counters) of fit() with the catalogue metrics inside it:
# tests/manual/catalogue_val_timing.py --trace, in a run of its own -- kernel trace for the kernels
# of an evaluation, HIP and memory-copy trace for what synchronises or copies between the first and
# last iteration of a fit -- and its summary (profiles/catalogue_val_trace_summary.py).  Run on the
# GPU box from the repository root:
#   profiles/catalogue_val_prof.sh [output directory (default: a fresh temporary one)] [timing options]
set -o pipefail
OUT=${1:-$(mktemp -d)}
shift
echo "output directory: $OUT"
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --hip-trace --memory-copy-trace --stats --output-format csv -d $OUT/catalogue_val_prof -- \
  python tests/manual/catalogue_val_timing.py --trace "$@" > $OUT/catalogue_val_prof.txt 2>&1 || { tail -20 $OUT/catalogue_val_prof.txt; exit 1; }
K=$(find $OUT/catalogue_val_prof -name "*kernel_trace.csv" | head -1)
A=$(find $OUT/catalogue_val_prof -name "*hip_api_trace.csv" | head -1)
M=$(find $OUT/catalogue_val_prof -name "*memory_copy_trace.csv" | head -1)
python profiles/catalogue_val_trace_summary.py "$K" $A $M | tee $OUT/catalogue_val_trace_summary.txt
