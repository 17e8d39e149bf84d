# host-side phase timings at the bench workload: setup (SSS_SETUP_TIMING) and upload (SSS_HIP_TIMING)
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
SSS_SETUP_TIMING=1 SSS_HIP_TIMING=${HIPT:-1} timeout -k 10 900 python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline \
  --converge-max 0 --parity-cycles 0 ${BENCH_ARGS} > $OUT/phases.json 2> $OUT/phases.err
rc=$?; grep -v "^ \|^---" $OUT/phases.err | tail -60; cat $OUT/phases.json | head -c 600; exit $rc
