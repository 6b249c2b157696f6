# one GPU-box pass for a round: SQ counters, HBM traffic, kernel-trace stats, then the bench lines (which quote the
# traffic / SQ profiles just taken: collect_profiles.py runs on the box first), the other BASELINE configs.
#   bash tools/gpu_bench_round.sh [TAG] [PART] [OUTDIR]        (from the repo root; outputs under OUTDIR, default prof_out)
# Afterwards, with OUTDIR copied back: python tools/collect_profiles.py TAG OUTDIR && python tools/design_numbers.py TAG
T=${1:-r06}
PART=${2:-ab}      # a: the counter / traffic / kernel-trace passes, collect, the bench line; b: the other bench lines and sweeps; ab: both
mkdir -p "${3:-prof_out}" && O=$(cd "${3:-prof_out}" && pwd) || exit 1
R=$(pwd)
if [[ $PART == *a* ]]; then
bash tools/prof_sq.sh $O/sq_${T} -1; rm -rf $O/sq_${T}/g*/
bash tools/prof_sq.sh $O/sq_${T}_f64 -1 harmonic 8 64; rm -rf $O/sq_${T}_f64/g*/
PVX_RUN_NFFT=4096 bash tools/prof_sq.sh $O/sq_${T}_nfft4096 -1; rm -rf $O/sq_${T}_nfft4096/g*/
PVX_RUN_NFFT=8192 bash tools/prof_sq.sh $O/sq_${T}_nfft8192 -1; rm -rf $O/sq_${T}_nfft8192/g*/
# the rest of the path, device to device, whole launches: tools/synth_time.py (analysis, pvx_track_dev, pvx_synth_dev x 3 on the C2 signal)
SYNTH_TIME_F32=1 SYNTH_TIME_NOCHECK=1 SYNTH_TIME_ONLY=harmonic PVX_PROF_PROG="tools/synth_time.py 600 3" bash tools/prof_sq.sh $O/sq_${T}_chain -1; rm -rf $O/sq_${T}_chain/g*/
bash tools/prof_traffic.sh $O/traffic_${T}; rm -rf $O/traffic_${T}/*_SIZE/
bash tools/prof_traffic.sh $O/traffic_${T}_f64 -1 harmonic 8 64; rm -rf $O/traffic_${T}_f64/*_SIZE/
SYNTH_TIME_F32=1 SYNTH_TIME_NOCHECK=1 SYNTH_TIME_ONLY=harmonic PVX_PROF_PROG="tools/synth_time.py 600 3" bash tools/prof_traffic.sh $O/traffic_${T}_chain; rm -rf $O/traffic_${T}_chain/*_SIZE/
# (rocprofv3 runs from a scratch directory: nothing it leaves behind lands in the tree)
(cd "$(mktemp -d)" && rocprofv3 --kernel-trace --stats -d "$O/stats_${T}" -o r --output-format csv -- python3 "$R/bench.py" --full --steps 20 --warmup 3 --no-extras --no-cpu-baseline --detail "$O/bench_stats_detail.json" > "$O/stats_${T}.log" 2>&1); ls $O/stats_${T}
python tools/collect_profiles.py ${T} $O > $O/collect_${T}.log 2>&1; echo "collect rc=$?"
python bench.py --full --detail $O/bench_${T}a_detail.json > $O/bench_${T}a.json 2> $O/bench_${T}a.err; echo "bench rc=$?"; tail -c 400 $O/bench_${T}a.err
fi
if [[ $PART == *b* ]]; then
PVX_BENCH_FORCE_GATHER=1 python bench.py --full --detail $O/bench_fg_detail.json --steps 5 --warmup 1 --no-extras --no-cpu-baseline > $O/bench_fg.json 2> $O/bench_fg.err; echo "forced gather rc=$?"
python bench.py --full --detail $O/bench_c4_detail.json --workload c4 --steps 5 --warmup 1 > $O/bench_c4.json 2> $O/bench_c4.err; echo "c4 rc=$?"; tail -2 $O/bench_c4.err
python tools/bench_configs.py > $O/configs_${T}.jsonl 2> $O/configs_${T}.err
python tools/sweep_config5.py > $O/sweep5_${T}.jsonl 2> $O/sweep5_${T}.err
python tools/sweep_config5.py 3600 64 > $O/sweep5_${T}_f64.jsonl 2>> $O/sweep5_${T}.err
python tools/ab_nfft.py 512,1024,2048,4096,8192 > $O/ab_nfft_${T}.jsonl 2>/dev/null
(cd "$(mktemp -d)" && rocprofv3 --kernel-trace --stats -d "$O/next_rows_${T}" -o r --output-format csv -- python3 "$R/tools/bench_next_rows.py" > "$O/next_rows_${T}.jsonl" 2> "$O/next_rows_${T}.err")
fi
