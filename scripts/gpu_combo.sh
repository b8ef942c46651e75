# parity (decoder + training), then decoder and training-step A/B: in-tree build vs lib_head.so
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 200 --timeout-method thread -k "train or persistent or parity or longhorizon" > $OUT/combo_tests.log 2>&1 || { echo "tests failed"; grep -E "FAILED|Error" $OUT/combo_tests.log | head -20; tail -30 $OUT/combo_tests.log; exit 1; }
tail -1 $OUT/combo_tests.log
for rep in 1 2; do
  for L in tree lib_head.so; do
    if [ "$L" = "tree" ]; then unset TT2_LIB; else export TT2_LIB=$GRAFT_REPO_ROOT/$L; fi
    timeout -k 10 200 python bench.py --full --steps 3 --warmup 1 --no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --no-variants --train-steps 3 > $OUT/cb.json 2> $OUT/cb.err || { echo "bench failed for $L"; tail -5 $OUT/cb.err; exit 1; }
    python -c "import json; d=json.loads(open('$OUT/cb.json').read().strip().splitlines()[-1]); print('$L', 'decode', d['phases']['decode_us_per_step'], 'train', d['train']['ms_per_step'], d['train']['loss_last'])"
  done
done
