#!/bin/bash
# kernel-trace stats of the generic device sampler on 1 250 HKY+Gamma4 loci (tools/closedform_rate.py): which kernels an
# iteration runs — no eigen_kernel, and the node-update kernel without its fused K6 phase.  Prints the rate line of an
# untraced run, then the head of the traced run's kernel statistics.   tools/trace_closedform.sh [hky|gtr] > trace_hky_1250.txt
R=$(cd "$(dirname "$0")/.." && pwd); M=${1:-hky}
W=$(mktemp -d); cd "$W" && export TMPDIR="$W"
timeout -k 10 200 python "$R/tools/closedform_rate.py" 1250 60 "$M" 2>/dev/null || { echo "rate run failed: $?"; exit 1; }
timeout -k 10 280 rocprofv3 --kernel-trace --stats -f csv -d "$W/trace" -o p -- python "$R/tools/closedform_rate.py" 1250 60 "$M" > /dev/null 2>&1 || { echo "trace run failed: $?"; exit 1; }
f=$(find "$W/trace" -name '*kernel_stats.csv' | head -1)
head -16 "$f" | cut -c1-160
echo "kernels with 'eigen' in their name: $(grep -c eigen "$f")"
