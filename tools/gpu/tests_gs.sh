# every -m gpu test, the per-level exact GS-CF times at 256^3 (flow engine), the throughput profile
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo tests failed; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python -u tools/gs_level_times.py --n 256 --engines flow --reps 3 --json $OUT/gs_levels.json > $OUT/gs_levels.txt 2>&1 || { tail -20 $OUT/gs_levels.txt; exit 1; }
grep "^\[gs\] flow" $OUT/gs_levels.txt
bash tools/gpu/prof.sh > $OUT/prof.out 2>&1 || { tail -20 $OUT/prof.out; exit 1; }
cat $OUT/prof_levels.txt
