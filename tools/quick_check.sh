#!/bin/bash
# GPU parity tests, then the full bench lines (secondary configs, host
# boundary and trace check; no CPU baseline) for the three single-GPU configs.
# Logs go to $OUT_DIR (default bench_out). Stops at the first failure; no retries.
O=${OUT_DIR:-bench_out}
export TMPDIR=/tmp; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/pt.log 2>&1 &&
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/q200.log 2> $O/q200.err &&
timeout -k 10 300 python bench.py --full --n 100 --no-cpu-baseline > $O/q100.log 2> $O/q100.err &&
timeout -k 10 300 python bench.py --full --n 256 --stencil 7 --steps 3 --no-cpu-baseline > $O/q7.log 2> $O/q7.err
