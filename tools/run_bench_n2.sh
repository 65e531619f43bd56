#!/bin/bash
# GPU-box helper: N=1 bench, then the N=2 bench path (2 ranks on the one GPU).
# Result lines and stderr go to $OUT (default: bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 > "$OUT/bench_n1.json" 2> "$OUT/bench_n1.err" || exit $?
timeout -k 10 600 python -u -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
    --master-port 29511 bench.py --gpus 2 --full --steps 10 --warmup 3 > "$OUT/bench_n2.json" 2> "$OUT/bench_n2.err"
