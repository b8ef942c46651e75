# rocprofv3 kernel-trace stats of the full default bench (decoder + WaveNet + E2E + Griffin-Lim legs)
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-full}
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG/trace -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $OUT/prof_$TAG.bench.json 2>/dev/null
echo rc=$?
