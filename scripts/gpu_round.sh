# full GPU cycle: parity tests, smoke, default bench, rocprof kernel-trace + PMC passes (tag = $1)
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-x}
timeout -k 10 1000 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > $OUT/tests_$TAG.log 2>&1 || { echo "tests failed"; tail -30 $OUT/tests_$TAG.log; exit 1; }
tail -2 $OUT/tests_$TAG.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo "bench failed"; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
bash scripts/gpu_prof.sh $TAG
