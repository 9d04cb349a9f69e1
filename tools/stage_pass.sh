#!/bin/bash
# per-stage counters of one single-stream SNUNet step: the three single-stream --pmc passes + the launch table + profiles/stage_traffic.py
# usage (GPU box): bash tools/stage_pass.sh <tag>   -> $OUT/<tag>_snunet_stage_traffic.json, <tag>_snunet_launch_map.json
set -u
TAG=${1:-r04}
R=${GRAFT_REPO_ROOT:-$(pwd)}
export OUT=${OUT:-$R/bench_out}    # output folder
cd /tmp && export TMPDIR=/tmp
export KSMI_OVERLAP_WGRAD=0 KSMI_OVERLAP_LANES=0
ARGS="--steps 4 --warmup 2 --no-cpu-baseline --no-solo"
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/prof_${TAG}_solo_fetch -o fetch -- python $R/bench.py $ARGS > $OUT/stage_${TAG}.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/prof_${TAG}_solo_write -o write -- python $R/bench.py $ARGS >> $OUT/stage_${TAG}.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --kernel-trace -d $OUT/prof_${TAG}_solo_mfma -o mfma -- python $R/bench.py $ARGS >> $OUT/stage_${TAG}.log 2>&1
BENCH_LAUNCH_MAP=$OUT/${TAG}_snunet_launch_map.json python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > /dev/null 2>> $OUT/stage_${TAG}.log
cd $R
python profiles/stage_traffic.py $OUT/prof_${TAG}_solo $OUT/${TAG}_snunet_launch_map.json $OUT/${TAG}_snunet_stage_traffic.json
rm -rf $OUT/prof_${TAG}_solo_fetch $OUT/prof_${TAG}_solo_write $OUT/prof_${TAG}_solo_mfma
