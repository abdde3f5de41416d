#!/bin/bash
# Kernel statistics of the descriptor export (bench_descriptor.py, 240x320, 16 pairs per step) and the forward /
# post-processing split.  Usage: tools/prof_descriptor.sh [out_dir]   (warm-up steps are profiled too: 2 + 8 steps)
set -euo pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/descriptor}
mkdir -p "$OUT"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT" -o run --output-format csv -- \
  python bench_descriptor.py --steps 8 --warmup 2 > "$OUT/bench_line.json"
STATS=$(find "$OUT" -name 'run_kernel_stats.csv' | head -1)
python tools/descriptor_kernel_split.py "$STATS" 10 | tee "$OUT/split.json"
