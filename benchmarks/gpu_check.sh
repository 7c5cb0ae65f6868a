#!/bin/bash
# One GPU call: the GPU test suite, smoke(), then optional extra steps, then the full bench.py run.
#   bash benchmarks/gpu_check.sh [tag] ["extra command"]      (results under $NBD_OUT_DIR, default bench_out/)
set -e
tag=${1:-head}
out=${NBD_OUT_DIR:-bench_out}
mkdir -p "$out"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$out/gputests_$tag.txt" 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > "$out/smoke_$tag.txt" 2>&1
if [ -n "$2" ]; then bash -c "$2"; fi
timeout -k 10 300 python bench.py --full > "$out/bench_$tag.json" 2> "$out/bench_$tag.err"
