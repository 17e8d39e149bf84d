# kernel-trace profile of a short bench run (N=1) + per-level breakdown of one V-cycle
set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
rm -rf $OUT/prof_cur
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_cur -o run --output-format rocpd csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --converge-max 0 --parity-cycles 0 ${BENCH_ARGS} > $OUT/prof_cur.log 2>&1 || { echo prof failed; tail -30 $OUT/prof_cur.log; exit 1; }
grep '^{' $OUT/prof_cur.log > $OUT/prof_bench.json
python3 tools/level_breakdown.py $(find $OUT/prof_cur -name '*.db' | head -1) $OUT/prof_bench.json | tee $OUT/prof_levels.txt
# per (kernel, workgroups): the level-0 launches of the roofline kernel apart from the other levels'
python3 tools/prof_summary.py $(find $OUT/prof_cur -name '*.db' | head -1) --shapes $OUT/prof_shapes.txt > /dev/null
