cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
bash tools/gpu/prof.sh > $OUT/prof.out 2>&1 || { tail -20 $OUT/prof.out; exit 1; }
cp $OUT/prof_levels.txt $OUT/prof_levels_400.txt; cp $OUT/prof_bench.json $OUT/prof_bench_400.json
timeout -k 10 400 python -u bench.py --full --workload circuit --no-cpu-baseline > $OUT/bench_circ.json 2> $OUT/bench_circ.err || { tail -20 $OUT/bench_circ.err; exit 1; }
head -c 300 $OUT/bench_circ.json; echo
tail -17 $OUT/prof_levels_400.txt
