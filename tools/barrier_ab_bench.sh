#!/bin/bash
# Development aid (GPU box): the default bench workload (AES-expanded, K = 32) under both barrier schedules, alternating builds.
set -eo pipefail
cd ${GRAFT_REPO_ROOT:-.}
LINE=$(mktemp)
for rep in 1 2; do
for F in "-DBCE_STEP_BARRIERS" ""; do
  BCE_EXTRA_FLAGS="$F" python openfhe-boolean-circuit-evaluator_amd/build.py --force > /dev/null
  python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$LINE" 2>/dev/null
  python -c "
import json, sys; d=json.load(open(sys.argv[1])); print('flags [$F]', round(d['value']), d['roofline']['avg_launch_ms'], d['config']['single_block_latency_s'])" "$LINE"
done
done
rm -f "$LINE"
