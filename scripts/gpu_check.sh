#!/bin/bash
# standard GPU cycle: parity tests, bench line, per-shape kernel durations (rocprofv3 kernel trace); results in $OUT
cd "$(dirname "$0")/.." && export TMPDIR=${TMPDIR:-/tmp}
TAG=${1:-chk}
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout 600 python -m pytest tests -m gpu -q -x 2>&1 | tail -3
timeout 600 python bench.py --steps 100 --warmup 10 --full --no-cpu-baseline 2>"$OUT/bench_err.log" > "$OUT/bench_$TAG.json"
python -c "
import json; d=json.load(open('$OUT/bench_$TAG.json')); r=d['roofline']
print('BENCH tok/s', d['value'], 'ms', d['ms_per_step'], 'chain GB/s', d['config']['chain_hbm_GBps'], '| gate/up', r['achieved'], 'GB/s', r['avg_launch_us'], 'us frac', r['frac'])"
rm -rf "$OUT/prof_$TAG"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -o $TAG -- python bench.py --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/prof_${TAG}_bench.json" 2>/dev/null
python scripts/trace_summary.py "$OUT/prof_$TAG/${TAG}_kernel_trace.csv" smallm
