# GPU-box: the round's evidence in one session: GPU tests, C3 and C5 benches, rocprofv3 trace + PMC
# passes over bench.py, then the default bench (with its CPU-baseline leg).  Usage: bash tools/gpu_final.sh TAG
set -o pipefail
TAG=${1:-final}
R=$(pwd); OUT=${DCX_OUT:-$R/bench_out}; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1
rc=$?; tail -2 $OUT/${TAG}_tests.log; [ $rc = 0 ] || exit $rc
timeout -k 10 400 python tools/c3_bench.py --kernels $OUT/${TAG}_c3_kernels > $OUT/${TAG}_c3.json 2> $OUT/${TAG}_c3.err || { echo C3_FAILED; exit 1; }
cat $OUT/${TAG}_c3.json
timeout -k 10 300 python tools/stream_bench.py --split-k 16 > $OUT/${TAG}_c5.json 2> $OUT/${TAG}_c5.err || { echo C5_FAILED; exit 1; }
cat $OUT/${TAG}_c5.json
bash tools/gpu_profile.sh $TAG || exit 1
DCX_BENCH_KERNELS=$OUT/${TAG}_bench_kernels.json timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo BENCH_FAILED; exit 1; }
cat $OUT/${TAG}_bench.json
