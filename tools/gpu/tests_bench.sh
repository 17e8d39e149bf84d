# every -m gpu test, then a bench run without the CPU baselines (quick V-cycle/s check)
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; tail -3 $OUT/gpu_tests.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error|error" $OUT/gpu_tests.log | head -30; exit $rc; }
timeout -k 10 600 python -u bench.py --full --no-cpu-baseline ${BENCH_ARGS} > $OUT/bench.json 2> $OUT/bench.err
rc=$?; cat $OUT/bench.json; [ $rc -eq 0 ] || tail -20 $OUT/bench.err; exit $rc
