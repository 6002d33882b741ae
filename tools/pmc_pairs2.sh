#!/bin/bash
# second set of SQ counter passes (instruction fetch, issue levels) over the config-2 bench
R=$(cd "$(dirname "$0")/.." && pwd); O=$(realpath -m "${OUT:-$R/build/prof}")/pmc_pu2; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
i=0
for set in "SQ_IFETCH SQ_IFETCH_LEVEL SQ_INSTS_SMEM SQ_ACTIVE_INST_MISC" "SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_LEVEL_WAVES SQ_WAVES" "SQ_BUSY_CU_CYCLES SQ_CYCLES SQ_WAVE_CYCLES SQ_THREAD_CYCLES_VALU"; do
  i=$((i+1))
  rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/p$i -o p$i -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $O/p$i.log 2>&1 || exit 1
done
echo ok
