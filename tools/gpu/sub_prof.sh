# the GPU tests of the tile/ELL kernels (parity, engines, distributed), then prof.sh
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_gs_engines.py tests/test_dist_gpu.py -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; tail -2 $OUT/gpu_tests.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error|assert" $OUT/gpu_tests.log | head -30; exit $rc; }
bash tools/gpu/prof.sh
