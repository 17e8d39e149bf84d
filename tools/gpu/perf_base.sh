# the default bench (as the driver runs it), then the SQ occupancy/stall pass
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 700 python -u bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err || { tail -30 $OUT/bench.err; exit 1; }
head -c 300 $OUT/bench.json; echo
bash tools/gpu/pmc_sq.sh
