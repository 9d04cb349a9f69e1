#!/bin/bash
# full evidence set of a round: bench lines (contract form) + rocprofv3 summaries for the model families
# usage (GPU box): bash tools/profile_all.sh <tag>      -> $OUT/<tag>_* ; copy what is to be judged into profiles/
TAG=${1:-r05}
R=${GRAFT_REPO_ROOT:-$(pwd)}
export OUT=${OUT:-$R/bench_out}    # output folder
mkdir -p $OUT
bash $R/tools/profile.sh ${TAG} > $OUT/prof_${TAG}.log 2>&1
cd /tmp && export TMPDIR=/tmp
for m in changeformer floodvit unet mae; do
  rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_${m}_stats -o stats -- python $R/bench.py --model $m --steps 3 --warmup 2 --no-cpu-baseline --no-solo > $OUT/prof_${TAG}_$m.log 2>&1
done
# HBM traffic counters of the other families (own passes: --pmc only with --kernel-trace; FETCH_SIZE and WRITE_SIZE do not fit one pass)
for m in changeformer floodvit unet mae; do
  rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/prof_${TAG}_${m}_fetch -o fetch -- python $R/bench.py --model $m --steps 3 --warmup 2 --no-cpu-baseline --no-solo >> $OUT/prof_${TAG}_$m.log 2>&1
  rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/prof_${TAG}_${m}_write -o write -- python $R/bench.py --model $m --steps 3 --warmup 2 --no-cpu-baseline --no-solo >> $OUT/prof_${TAG}_$m.log 2>&1
done
# MFMA-busy counters (own pass)
for m in changeformer floodvit unet mae; do
  rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --kernel-trace -d $OUT/prof_${TAG}_${m}_mfma -o mfma -- python $R/bench.py --model $m --steps 3 --warmup 2 --no-cpu-baseline --no-solo >> $OUT/prof_${TAG}_$m.log 2>&1
done
cd $R
python profiles/summarize.py $OUT/prof_${TAG} $OUT/${TAG}_snunet_summary.md "SNUNet-ECAM bs=32 bf16 train step on THREE HIP streams (kernel durations overlap: their sum exceeds the step; single-stream durations and counters: ${TAG}_snunet_solo_summary.md)" "python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-solo" $OUT/${TAG}_snunet_traffic.json >> $OUT/prof_${TAG}.log 2>&1
python profiles/summarize.py $OUT/prof_${TAG}_solo $OUT/${TAG}_snunet_solo_summary.md "SNUNet-ECAM bs=32 bf16 train step on ONE stream (KSMI_OVERLAP_WGRAD=0 KSMI_OVERLAP_LANES=0)" "KSMI_OVERLAP_WGRAD=0 KSMI_OVERLAP_LANES=0 python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-solo" $OUT/${TAG}_snunet_solo_traffic.json >> $OUT/prof_${TAG}.log 2>&1
# per-stage counted traffic / MFMA-busy of one single-stream step: per-dispatch PMC rows aligned with the launch table of the same plan
KSMI_OVERLAP_WGRAD=0 KSMI_OVERLAP_LANES=0 BENCH_LAUNCH_MAP=$OUT/${TAG}_snunet_launch_map.json python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline > /dev/null 2>> $OUT/prof_${TAG}.log
python profiles/stage_traffic.py $OUT/prof_${TAG}_solo $OUT/${TAG}_snunet_launch_map.json $OUT/${TAG}_snunet_stage_traffic.json >> $OUT/prof_${TAG}.log 2>&1
for m in changeformer floodvit unet mae; do
  python profiles/summarize.py $OUT/prof_${TAG}_$m $OUT/${TAG}_${m}_summary.md "$m train step (bench.py --model $m)" "python bench.py --model $m --steps 3 --warmup 2 --no-cpu-baseline --no-solo" $OUT/${TAG}_${m}_traffic.json >> $OUT/prof_${TAG}.log 2>&1
done
# the bench lines (contract form) last: roofline.traffic is read from the per-kernel tables the passes above just produced
cp $OUT/${TAG}_*_traffic.json profiles/ 2>/dev/null
python $R/bench.py --full > $OUT/${TAG}_bench_snunet.json 2> $OUT/${TAG}_bench.err
for m in changeformer floodvit unet mae siam-conc siam-diff bit-cd; do python $R/bench.py --full --model $m --no-cpu-baseline > $OUT/${TAG}_bench_$m.json 2>> $OUT/${TAG}_bench.err; done
python $R/bench.py --full --model changeformer --channels 4 --no-cpu-baseline > $OUT/${TAG}_bench_changeformer_slc.json 2>> $OUT/${TAG}_bench.err
python $R/profiles/stream_probe.py 2>&1 | grep MiB > $OUT/${TAG}_stream_probe.txt
python $R/profiles/gemm_probe.py 2>&1 | grep rows > $OUT/${TAG}_gemm_probe.txt
python $R/tools/gemm_durations.py $OUT/prof_${TAG}_floodvit_stats/stats_results.db > $OUT/${TAG}_floodvit_gemm_durations.txt 2>&1
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29519 $R/bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-solo > $OUT/${TAG}_torchrun_stdout.txt 2> $OUT/${TAG}_torchrun_stderr.txt
# the raw rocpd databases are tens of MiB each: keep the summaries, drop the databases
rm -rf $OUT/prof_${TAG}_*_fetch $OUT/prof_${TAG}_*_write $OUT/prof_${TAG}_solo_stats $OUT/prof_${TAG}_stats $OUT/prof_${TAG}_fetch $OUT/prof_${TAG}_write $OUT/prof_${TAG}_mfma $OUT/prof_${TAG}_*_stats $OUT/prof_${TAG}_*_mfma
du -sh $OUT; ls $OUT | grep ${TAG}_ | head -40
