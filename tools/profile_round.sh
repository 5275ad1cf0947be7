#!/bin/bash
# Developer helper (GPU box): the evidence set for profiles/ -- the full bench line, rocprofv3 kernel stats of the same
# command, and the HBM-traffic counters (separate --pmc pass).  Usage: tools/profile_round.sh TAG [OUT_DIR]
# Everything goes to OUT_DIR (default: profile_out/ in the repository, git-ignored); tools/hbm_traffic.py TAG OUT_DIR reads it.
set -e
TAG=${1:-vX}
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${2:-$R/profile_out}" && cd "${2:-$R/profile_out}" && pwd)
[ -n "$SKIP_BENCH" ] || python3 $R/bench.py --full --steps 20 --warmup 5 > $O/bench_$TAG.json 2> $O/bench_$TAG.err
cd /tmp && export TMPDIR=/tmp
[ -n "$SKIP_BENCH" ] || rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_$TAG -- python3 $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-secondary > $O/stats_$TAG.log 2>&1
# FETCH_SIZE and WRITE_SIZE do not fit one pass ("exceeds the capabilities of the hardware"): one pass each
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 5 150 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $O/pmc_${c}_$TAG -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $O/pmc_${c}_$TAG.log 2>&1
done
echo profiled $TAG
