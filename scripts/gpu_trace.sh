# kernel-trace only (tag = $1), decoder bench
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-tr}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/trace_$TAG -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-wavenet > $OUT/trace_$TAG.json 2>/dev/null
echo rc=$?
head -20 $OUT/trace_$TAG/run_kernel_stats.csv | cut -d, -f1-4
