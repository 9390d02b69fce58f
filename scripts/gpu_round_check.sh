#!/bin/bash
# Full GPU check of the tree on one MI355X: every GPU test, the full bench line (every section with its checks), and
# a rocprofv3 kernel-stats profile of a short full bench run (summaries go to <out>/<tag>_*; copy the ones to keep
# into profiles/).
# usage: scripts/gpu_round_check.sh <tag> [out-dir, default build/check]
set -o pipefail
tag=${1:-check}
out=${2:-build/check}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 660 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $out/${tag}_gputest.log 2>&1 &&
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $out/${tag}_bench.log 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -o bench -- \
  python3 bench.py --full --steps 5 --warmup 2 --no-ref > $out/${tag}_bench_rocprof.log 2>&1
