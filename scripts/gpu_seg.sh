# round 3: the rocprofv3 exit segfault with cooperative launches -- exit guard, then a PMC pass
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the output directory of this run}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_seg -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-wavenet --no-e2e --no-griffin-lim --no-variants > $OUT/seg.out 2> $OUT/seg.err
echo "prof coop+guard rc=$?"
tail -2 $OUT/seg.err; ls -la $OUT/prof_seg
timeout -k 10 120 rocprofv3 --pmc WRITE_SIZE -d $OUT/prof_seg_w -o run --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-wavenet --no-e2e --no-griffin-lim --no-variants --no-train > $OUT/segw.out 2> $OUT/segw.err
echo "pmc coop+guard rc=$?"
ls -la $OUT/prof_seg_w
