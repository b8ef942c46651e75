# 256-thread attention energy kernels: training parity, A/B (TT2_TR_E2), kernel stats
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest tests/test_train.py tests/test_train_options.py -x -q -m gpu --timeout 150 --timeout-method thread > $OUT/e2_tests.log 2>&1 || { echo "tests failed"; tail -40 $OUT/e2_tests.log; exit 1; }
tail -2 $OUT/e2_tests.log
for cfg in "TT2_TR_E2=1" "TT2_TR_E2=0" "TT2_TR_E2=1"; do
  env $cfg timeout -k 10 200 python bench.py --full --steps 1 --warmup 1 --no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --no-variants > $OUT/e2_t.json 2> $OUT/e2_t.err || { echo "train bench failed"; tail -5 $OUT/e2_t.err; exit 1; }
  python -c "import json; d=json.loads(open('$OUT/e2_t.json').read().strip().splitlines()[-1]); print('$cfg train ms', d['train']['ms_per_step'], d['train']['loss_first'], d['train']['grad_norm'])"
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_e2 -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --no-variants > $OUT/e2_prof.json 2> $OUT/e2_prof.err || { echo "prof failed"; tail -5 $OUT/e2_prof.err; exit 1; }
grep -E "att_|tr_ctx" $OUT/prof_e2/run_kernel_stats.csv | cut -d, -f1-4 | cut -c1-110
