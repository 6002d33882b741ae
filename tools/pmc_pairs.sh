#!/bin/bash
# SQ counter passes over the config-2 bench (one rocprofv3 --pmc run per counter set, kernel trace only).
# Run on the MI355X: bash tools/pmc_pairs.sh ; results under $OUT/pmc_pu/ (OUT: build/prof by default)
R=$(cd "$(dirname "$0")/.." && pwd); O=$(realpath -m "${OUT:-$R/build/prof}")/pmc_pu; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_ANY" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_BRANCH" "SQ_WAIT_INST_LDS SQ_INST_CYCLES_SALU SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD"; do
  i=$((i+1))
  rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/p$i -o p$i -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/p$i.log 2>&1 || exit 1
done
echo ok
