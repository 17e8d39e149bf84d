# Whole GPU check: every -m gpu test, 256^3 parity/throughput histories, default bench.
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; tail -4 $OUT/gpu_tests.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error" $OUT/gpu_tests.log | head -20; exit $rc; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; tail -2 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
if [ -n "$CONV" ]; then
timeout -k 10 600 python -u tools/conv_study.py --n 256 --modes $CONV --maxit 40 --json $OUT/conv256.json > $OUT/conv256.log 2>&1
rc=$?; grep "\[conv\].*iterations" $OUT/conv256.log; [ $rc -eq 0 ] || exit $rc
fi
if [ -n "$BENCH" ]; then
timeout -k 10 900 python -u bench.py --full $BENCH_ARGS > $OUT/bench.json 2> $OUT/bench.err
rc=$?; cat $OUT/bench.json; [ $rc -eq 0 ] || { tail -20 $OUT/bench.err; exit $rc; }
fi
