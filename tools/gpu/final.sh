# Round-end evidence on one GPU: level-0 PMC (CSR arrays and the cycle's storage) into profiles/,
# smoke, then the default bench (it reads the PMC file for roofline.traffic), then the kernel-trace
# profile of the same command with its per-level split.
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
bash tools/gpu/pmc.sh || exit 1
python3 tools/pmc_summarize.py $OUT profiles/r02_level0_spmv_pmc.json > /dev/null || exit 1
cp profiles/r02_level0_spmv_pmc.json $OUT/level0_spmv_pmc.json
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; tail -2 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python -u bench.py --full $BENCH_ARGS > $OUT/bench.json 2> $OUT/bench.err
rc=$?; cat $OUT/bench.json; [ $rc -eq 0 ] || { tail -20 $OUT/bench.err; exit $rc; }
bash tools/gpu/prof.sh
# N = 2 on the one-GPU box: two ranks (host transport when RCCL cannot pair two ranks on one GPU)
timeout -k 10 300 python -u bench.py --full --gpus 2 --n 64 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_g2.json 2> $OUT/bench_g2.err
rc=$?; tail -c 400 $OUT/bench_g2.json; exit $rc
