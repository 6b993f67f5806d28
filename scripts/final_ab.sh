# same-box lines: HIP engine (RAFT, RAFT-small) and the stock-PyTorch A/B (both graphed for inference)
OUT=${OUT:-out}  # where logs and profiles go
mkdir -p $OUT/final
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $OUT/final/hip.log 2>&1 && tail -1 $OUT/final/hip.log && \
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --small > $OUT/final/small.log 2>&1 && tail -1 $OUT/final/small.log && \
timeout -k 10 400 python bench.py --full --steps 5 --warmup 2 --reference-ops > $OUT/final/ref.log 2>&1 && tail -1 $OUT/final/ref.log
