#!/bin/bash
# A/B of environment switches on one box: tools/ab_bench.sh "VAR=1" "VAR=2" ... (each run: 12 timed steps, eager).
# Every arm runs under its own time limit; the first arm that fails ends the script (nothing more is started on the GPU).
set -o pipefail
for cfg in "$@"; do
  echo "== $cfg"
  env $cfg timeout -k 10 300 python bench.py --launch eager --no-extra-modes --no-cpu-baseline --no-kernel-events --steps 12 2>/dev/null |
    python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['ms_per_step'], d['ms_per_step_median'], d.get('loss'))" || exit 1
done
