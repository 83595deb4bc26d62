#!/bin/bash
# Run ON THE GPU BOX (via gpurun): bench + rocprofv3 kernel trace + separate PMC passes for HBM traffic.
# Outputs go to $OUT (default out/); summaries are produced afterwards by tools/rocprof_summary.py / tools/pmc_summary.py.
set -u
R=$PWD
O=${OUT:-$R/out}
mkdir -p $O
timeout 900 python bench.py --full > $O/bench.json 2> $O/bench.err
cat $O/bench.json
cd /tmp && export TMPDIR=/tmp
rm -rf $O/trace $O/pmc_fetch $O/pmc_write $O/pmc_sq
timeout 600 rocprofv3 --kernel-trace --stats -d $O/trace -o t -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --bf16x3-steps 0 --single-steps 0 --inflight-steps 0 --other-configs-steps 0 > $O/trace.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch -o p -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --bf16x3-steps 0 --single-steps 0 --inflight-steps 0 --other-configs-steps 0 --unique 64 > $O/pmc_fetch.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write -o p -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --bf16x3-steps 0 --single-steps 0 --inflight-steps 0 --other-configs-steps 0 --unique 64 > $O/pmc_write.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_MFMA GRBM_GUI_ACTIVE -d $O/pmc_sq -o p -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --bf16x3-steps 0 --single-steps 0 --inflight-steps 0 --other-configs-steps 0 --unique 64 > $O/pmc_sq.log 2>&1
ls $O
cd $R
timeout 600 python tools/latency.py > $O/latency.txt 2>&1
for f in "" "--sparse" "--sparse --gpu-graph" "--device-explore --problems 1024" "--device-explore --device-smooth --problems 1024"; do
  timeout 600 python tools/planner_bench.py $f 2>/dev/null | tail -1
done > $O/planner_bench.txt
timeout 300 python bench.py --full --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --dense-steps 0 --bf16x3-steps 0 --single-steps 0 --inflight-steps 0 --other-configs-steps 0 --env kuka7 --nodes 2000 --k1 10 --graphs 64 --mlp-dtype bf16 2>/dev/null | tail -1 > $O/bench_cfg3_kuka7_bf16.json
timeout 300 python bench.py --full --no-cpu-baseline --planner-problems 0 --pcie-steps 0 --dense-steps 0 --mlp-dtype bf16x3 2>/dev/null | tail -1 > $O/bench_cfg2_bf16x3.json
ls $O
