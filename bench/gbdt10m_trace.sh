#!/bin/bash
# GBDT 20 trees x depth 6 on 10M rows (the bench.py headline training shape): kernel trace split
# per boosting round (bench/trace_rounds.py).
# Usage: bash bench/gbdt10m_trace.sh <tag>
set -e
TAG=${1:-g10m}
OUT=gpurun_out/$TAG
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_native" -o run -- \
  python3 bench/gbdt_train.py --rows 10000000 --trees 20 > "$OUT/native.json" 2> "$OUT/native.err"
tail -1 "$OUT/native.json" | cut -c1-300
TR=$(find "$OUT/prof_native" -name "*kernel_trace.csv" | head -1)
python bench/trace_rounds.py "$TR" --round 10 > "$OUT/rounds_native.txt" 2>&1 || true
head -14 "$OUT/rounds_native.txt"; sed -n '/^ *[0-9.]* ms  *[0-9]*  /p' "$OUT/rounds_native.txt" | head -16
rm -f "$TR"
