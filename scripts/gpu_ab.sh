# A/B decoder timing: bench.py decoder leg under each library build given as args (in-tree = "tree")
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
for rep in 1 2; do
  for L in "$@"; do
    if [ "$L" = "tree" ]; then unset TT2_LIB; else export TT2_LIB=$GRAFT_REPO_ROOT/$L; fi
    timeout -k 10 120 python bench.py --full --steps 3 --warmup 1 --no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --no-train --no-variants > $OUT/ab.json 2> $OUT/ab.err || { echo "bench failed for $L"; tail -5 $OUT/ab.err; exit 1; }
    python -c "import json,sys; d=json.loads(open('$OUT/ab.json').read().strip().splitlines()[-1]); print('$L', d['phases']['decode_us_per_step'], d['value'])"
  done
done
