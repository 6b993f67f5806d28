#!/bin/bash
# Tune RAFT-small's bf16 inference calls at the Sintel bench shape
# (1088x436), then measure bench.py --small (paired with the old table).
set -o pipefail
OUT=${OUT:-out}  # where logs and profiles go
mkdir -p $OUT/tsi
export HSA_ENABLE_IPC_MODE_LEGACY=0
cp raft_stir_amd/conv_tuning.json $OUT/tsi/conv_tuning.json
cp raft_stir_amd/conv_tuning.json $OUT/tsi/conv_tuning_old.json
timeout -k 10 300 python scripts/tune_conv.py --small --infer-only --merge --out $OUT/tsi/conv_tuning.json > $OUT/tsi/tune.log 2>&1 || { tail -20 $OUT/tsi/tune.log; exit 1; }
tail -n 1 $OUT/tsi/tune.log
for t in new old new old; do
  if [[ $t == new ]]; then cp $OUT/tsi/conv_tuning.json raft_stir_amd/conv_tuning.json; else cp $OUT/tsi/conv_tuning_old.json raft_stir_amd/conv_tuning.json; fi
  timeout -k 10 300 python bench.py --full --small --steps 10 --warmup 5 --infer-reps 50 > $OUT/tsi/b.log 2>&1 || { tail -20 $OUT/tsi/b.log; exit 1; }
  echo "$t $(tail -1 $OUT/tsi/b.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["inference"]["fps"])')"
done
