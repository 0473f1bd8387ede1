# GPU-box: rocprofv3 kernel trace + FETCH/WRITE PMC passes over bench.py.  Usage: bash tools/gpu_profile.sh TAG
set -o pipefail
TAG=${1:-prof}
R=$(pwd); OUT=${DCX_OUT:-$R/bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
cd $R
DCX_BENCH_KERNELS=$OUT/${TAG}_kernels.json timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_trace -o run --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-f32 --no-c3 --no-c4 --no-c5 --no-oracle-codes > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_trace.err || { echo TRACE_FAILED; exit 1; }
echo TRACE_OK
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/${TAG}_fetch -o run --output-format csv -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-f32 --no-profile --no-c3 --no-c4 --no-c5 --no-oracle-codes > /dev/null 2> $OUT/${TAG}_fetch.err || { echo FETCH_FAILED; exit 1; }
echo FETCH_OK
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/${TAG}_write -o run --output-format csv -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-f32 --no-profile --no-c3 --no-c4 --no-c5 --no-oracle-codes > /dev/null 2> $OUT/${TAG}_write.err || { echo WRITE_FAILED; exit 1; }
echo WRITE_OK
python3 tools/pmc_to_json.py $OUT/${TAG}_fetch $OUT/${TAG}_write > $OUT/${TAG}_pmc.json
python3 tools/rocprof_summary.py --stats $(ls $OUT/${TAG}_trace/*kernel_stats.csv $OUT/${TAG}_trace/*/*kernel_stats.csv 2>/dev/null | head -1) --fetch $(find $OUT/${TAG}_fetch -name "*counter_collection.csv" | head -1) --write $(find $OUT/${TAG}_write -name "*counter_collection.csv" | head -1) --bench-kernels $OUT/${TAG}_kernels.json > $OUT/${TAG}_summary.md
head -12 $OUT/${TAG}_summary.md
