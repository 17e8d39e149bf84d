# every -m gpu test, then the kernel-trace profile of a short bench with its per-level split
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gpu_tests.log 2>&1 || { echo tests failed; tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
bash tools/gpu/prof.sh > $OUT/prof.out 2>&1 || { tail -20 $OUT/prof.out; exit 1; }
cat $OUT/prof_levels.txt
