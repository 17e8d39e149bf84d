# every -m gpu test, then the per-level kernel profile of the bench workload (prof.sh)
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 500 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; tail -3 $OUT/gpu_tests.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error|assert" $OUT/gpu_tests.log | head -30; exit $rc; }
bash tools/gpu/prof.sh
