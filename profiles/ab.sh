#!/bin/bash
# A/B helper: bash profiles/ab.sh <tag> [ENV=VAL ...]  -> kernel stats of one bench run under rocprofv3
#   (bench.py --full: the extra measurements' launches are part of the stats; written under $OUT, default profiles/out)
set -eo pipefail
TAG=$1; shift
R=$(pwd)
OUT=${OUT:-$R/profiles/out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for kv in "$@"; do export "$kv"; done
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ab_$TAG" -o ab -- \
  python3 "$R/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/ab_$TAG.log" 2>&1
cd "$R"
echo "== $TAG $*"
grep -o '"ms_per_step": [0-9.]*' "$OUT/ab_$TAG.log" || true
python3 profiles/summarize_stats.py "$OUT/ab_$TAG" 14
