set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 && \
timeout -k 10 600 python bench.py --full --steps 3 --warmup 1 > $OUT/bench1.json 2> $OUT/bench1.err && \
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof1 -o run --output-format csv -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/bench_prof1.json 2> $OUT/bench_prof1.err
echo rc=$?
