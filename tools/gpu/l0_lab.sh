# level-0 rows-per-thread lab (tools/l0_lab.hip, prebuilt in-tree), then the distributed GPU tests
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 300 ./tools/l0_lab 400 20 > $OUT/l0_lab.txt 2>&1 || { cat $OUT/l0_lab.txt; exit 1; }
cat $OUT/l0_lab.txt
timeout -k 10 600 python -u -m pytest tests/test_dist_gpu.py -x -v --timeout 120 --timeout-method thread > $OUT/dist_gpu.log 2>&1
rc=$?; tail -25 $OUT/dist_gpu.log; exit $rc
