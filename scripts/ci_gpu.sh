#!/bin/bash
# Standard GPU validation batch; run from the repo root on an MI355X box:
#   bash scripts/ci_gpu.sh
# Produces logs under ci_out/ (override with CI_OUT=<dir>).
# Every step has its own time limit and the batch stops at the first
# failing step, so nothing more is started on a GPU that just faulted.
set -euo pipefail
out="${CI_OUT:-ci_out}"
mkdir -p "$out"

echo "== pytest -m gpu =="
timeout -k 10 1200 python -m pytest tests -m gpu -q 2>&1 | tail -2

echo "== smoke =="
timeout -k 10 90 python -c "import __graft_entry__; __graft_entry__.smoke()" 2>&1 | tail -1

echo "== bench (10M default config) =="
timeout -k 10 240 python bench.py --gpus 1 --steps 3 --warmup 1 2>&1 \
    | grep -E "^\{|stage timings" | tee "$out/bench.json"

echo "== kernel profile (2M short run) =="
timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof" -o ci \
    -- python bench.py --rows 2000000 --steps 1 --warmup 1 \
       --min-warmup-seconds 4 > "$out/rocprof.log" 2>&1
ls "$out/prof"
