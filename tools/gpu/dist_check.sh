# every -m gpu test, then bench.py --gpus 2 on the one GPU (two ranks, host transport fallback)
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; tail -3 $OUT/gpu_tests.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error|error" $OUT/gpu_tests.log | head -30; exit $rc; }
SSS_PART_DIR=$PWD/$OUT/parts timeout -k 10 600 python -u bench.py --full --gpus 2 --n 64 --steps 5 --warmup 2 > $OUT/bench2.json 2> $OUT/bench2.err
rc=$?; cat $OUT/bench2.json; tail -5 $OUT/bench2.err; rm -rf $OUT/parts; exit $rc
