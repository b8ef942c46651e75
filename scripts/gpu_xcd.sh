# decoder stage stamps of step 500 over several launches: which physical XCD (HW_REG_XCC_ID) runs slow
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
O=$OUT/$1
mkdir -p $O
export TMPDIR=/tmp
for k in 1 2 3; do
  TT2_STAMP_OUT=$OUT/pd_stamps.npy TT2_STAMP_STEP=500 timeout -k 10 300 python -u bench.py --full --steps 1 --warmup 1 --no-wavenet --no-e2e --no-griffin-lim --no-cpu-baseline --no-variants --no-train > $O/stamps$k.json 2> $O/stamps$k.err || { echo "stamp bench failed"; tail -5 $O/stamps$k.err; exit 1; }
  cp $OUT/pd_stamps.npy $O/pd_stamps$k.npy && python scripts/stamps.py $O/pd_stamps$k.npy | tail -9
done
