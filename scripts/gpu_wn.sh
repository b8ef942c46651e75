# WaveNet-only GPU cycle: parity tests + generation bench (tag = $1)
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-w}
timeout -k 10 300 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "wavenet or mol" > $OUT/wn_tests_$TAG.log 2>&1 || { echo "tests failed"; tail -40 $OUT/wn_tests_$TAG.log; exit 1; }
tail -2 $OUT/wn_tests_$TAG.log
timeout -k 10 300 python bench.py --full --steps 1 --warmup 1 --t-out 50 --no-cpu-baseline --profile-iters 5 > $OUT/wn_bench_$TAG.json 2> $OUT/wn_bench_$TAG.err || { echo "bench failed"; tail -20 $OUT/wn_bench_$TAG.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/wn_bench_$TAG.json')); print(json.dumps(d['wavenet']))"
