#!/bin/bash
# kernel-trace stats of the generic sampler on one config
R=${GRAFT_REPO_ROOT:-$(pwd)}; CFG=${1:-c3}
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/tr0
timeout 280 rocprofv3 --kernel-trace --stats -f csv -d /tmp/tr0 -o p -- python $R/bench.py --config $CFG --no-tape --no-scale-projection --no-other-configs --no-cpu-baseline --no-host-control --no-bpp-program --no-efficiency > /dev/null 2>&1
echo "== $CFG"; f=$(find /tmp/tr0 -name '*kernel_stats.csv' | head -1); head -9 "$f" | cut -c1-200
