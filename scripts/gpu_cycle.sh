# one GPU cycle: parity tests, smoke, bench (tag = $1)
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-x}
timeout -k 10 900 python -m pytest tests -x -q -m gpu > $OUT/tests_$TAG.log 2>&1 || { echo "tests failed"; tail -30 $OUT/tests_$TAG.log; exit 1; }
tail -2 $OUT/tests_$TAG.log
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 ${BENCH_ARGS} > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo "bench failed"; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
