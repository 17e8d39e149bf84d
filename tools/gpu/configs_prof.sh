# the other BASELINE workloads on one GPU at HEAD: G3_circuit stand-in and 27-pt anisotropic 256^3 bench
# lines, each with a kernel-trace profile split per level
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
timeout -k 10 600 python -u bench.py --full --workload circuit --no-cpu-baseline > $OUT/bench_circuit.json 2> $OUT/bench_circuit.err || { tail -20 $OUT/bench_circuit.err; exit 1; }
head -c 300 $OUT/bench_circuit.json; echo
BENCH_ARGS="--workload circuit" bash tools/gpu/prof.sh > /dev/null && cp $OUT/prof_levels.txt $OUT/circuit_levels.txt
tail -14 $OUT/circuit_levels.txt
timeout -k 10 900 python -u bench.py --full --stencil 27 --n 256 --no-cpu-baseline --parity-cycles 0 > $OUT/bench_a27.json 2> $OUT/bench_a27.err || { tail -20 $OUT/bench_a27.err; exit 1; }
head -c 300 $OUT/bench_a27.json; echo
