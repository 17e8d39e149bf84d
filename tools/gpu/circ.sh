# circuit workload: its GPU tests, the free-order/parity suites the changes touch, a bench line
# and a per-level kernel profile
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -x -q -s --timeout 500 --timeout-method thread -m gpu > $OUT/tc.log 2>&1
rc=$?; grep -E "circuit 1.58M|passed|failed|FAIL|Error" $OUT/tc.log | head -20; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full --workload circuit > $OUT/bench_circ.json 2> $OUT/bench_circ.err || { tail -20 $OUT/bench_circ.err; exit 1; }
cat $OUT/bench_circ.json
BENCH_ARGS="--workload circuit" bash tools/gpu/prof.sh
