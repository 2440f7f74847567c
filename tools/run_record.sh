# Round record run (one gpurun call): PMC traffic of the final sources first (so that bench.py's roofline.traffic carries a
# matching fingerprint), then the `bench.py --full` line, the rocprofv3 kernel statistics of the same command, episode and
# reprojection benches, per-shape breakdown -> floor table (true-peak + yardstick columns, vendor rates of the same call), effective clock.
# Usage on the GPU box: bash tools/run_record.sh <tag>   (tag e.g. r06_d; outputs in $EW_RECORD_DIR/<tag>_*, default records/, copied to profiles/ by hand)
set -x
R=$GRAFT_REPO_ROOT
T=${1:-r06_x}
export EW_ROUND=${T%%_*}
O=${EW_RECORD_DIR:-$R/records}; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
bash $R/tools/pmc_traffic.sh > $O/${T}_hbm_traffic.txt 2>&1
tail -3 $O/${T}_hbm_traffic.txt
cp $R/gpurun_out/${EW_ROUND}_hbm_traffic.json $R/profiles/${EW_ROUND}_hbm_traffic.json
bash $R/tools/pmc_clock.sh $EW_ROUND > $O/${T}_effective_clock.txt 2>&1; tail -12 $O/${T}_effective_clock.txt
cp $R/gpurun_out/${EW_ROUND}_clock.json $R/profiles/${EW_ROUND}_clock.json
cd $R
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
tail -c 900 $O/${T}_bench.json
cd $TMPDIR
rm -rf $TMPDIR/prof_f
rocprofv3 --kernel-trace --stats --output-format csv -d $TMPDIR/prof_f -- python $R/bench.py --full --steps 1 --warmup 0 --denoise-steps 2 --no-cpu-baseline --no-fp16-stream > $TMPDIR/prof_f.log 2>&1
f=$(find $TMPDIR/prof_f -name "*kernel_trace.csv" | head -1)
python $R/tools/csv_kernel_stats.py $f 3 > $O/${T}_three_forwards_kernel_stats.md
python $R/tools/steady_state_forward.py $f > $O/${T}_steady_state_forward.md 2>&1; head -6 $O/${T}_steady_state_forward.md
s=$(find $TMPDIR/prof_f -name "*kernel_stats.csv" | head -1)
[ -n "$s" ] && head -40 $s > $O/${T}_rocprofv3_kernel_stats.csv
head -12 $O/${T}_three_forwards_kernel_stats.md
cd $R
python bench_episode.py > $O/${T}_bench_episode.json 2> $O/${T}_bench_episode.err; tail -c 700 $O/${T}_bench_episode.json; tail -3 $O/${T}_bench_episode.err
python bench_reproject.py > $O/${T}_bench_reproject.json 2> $O/${T}_bench_reproject.err; tail -c 900 $O/${T}_bench_reproject.json
timeout 600 python tools/experiments/exp30_vs_hipblaslt.py > $O/${T}_vs_hipblaslt.txt 2>&1
EW_BENCH_FULL_BREAKDOWN=1 EW_BENCH_BY_SHAPE=1 python bench.py --full --steps 1 --warmup 1 --denoise-steps 4 --no-cpu-baseline --no-fp16-stream > $O/${T}_bd.json 2> $O/${T}_bd.txt
CLK=$(python -c "import bench; print(round(bench.committed_clock()['ghz'], 3))" 2>/dev/null)     # time-weighted over the launches of >= 300 us (short ones read high)
python tools/floor_table.py $O/${T}_bd.txt ${CLK:+--clock $CLK} --vendor $O/${T}_vs_hipblaslt.txt > $O/${T}_floor_table.md; tail -12 $O/${T}_floor_table.md
