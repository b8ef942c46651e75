# training leg: bench (configs[4]) + rocprof kernel stats (tag = $1)
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-x}
ARGS="--no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --steps 1 --warmup 1 ${TRAIN_ARGS}"
timeout -k 10 600 python bench.py --full $ARGS > $OUT/train_$TAG.json 2> $OUT/train_$TAG.err || { echo "bench failed"; tail -20 $OUT/train_$TAG.err; exit 1; }
python -c "import json; d=json.load(open('$OUT/train_$TAG.json')); print(json.dumps(d['train']))"
if [ -n "$PROF" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_train_$TAG -o run --output-format csv -- python bench.py --full $ARGS --train-steps 1 > $OUT/train_prof_$TAG.json 2> $OUT/train_prof_$TAG.err || { echo "prof failed"; tail -20 $OUT/train_prof_$TAG.err; exit 1; }
fi
echo done
