#!/bin/bash
# kernel stats of one bench configuration: bash profiles/stats_config.sh <tag> <bench args...>
#   -> $OUT/<tag>_stats/ (rocprofv3 --kernel-trace --stats), $OUT/<tag>_bench.log; $OUT defaults to profiles/out
#   (bench.py --full: the extra measurements' launches are part of the stats)
set -eo pipefail
TAG=$1; shift
R=$(pwd)
OUT=${OUT:-$R/profiles/out}
mkdir -p "$OUT"
export TMPDIR=/tmp
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_stats" -o st -- \
  python3 "$R/bench.py" --full --no-cpu-baseline "$@" > "$OUT/${TAG}_bench.log" 2>&1
cd "$R"
grep -o '"ms_per_step": [0-9.]*' "$OUT/${TAG}_bench.log" || true
python3 profiles/summarize_stats.py "$OUT/${TAG}_stats" 25
