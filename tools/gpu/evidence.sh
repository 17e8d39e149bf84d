# Evidence at HEAD on one GPU lease (ROUND, default r04; COMMIT stamped into the PMC file):
#  1. level-0 PMC traffic of both storages -> profiles/${ROUND}_level0_spmv_pmc.json (the bench reads
#     the newest such file for roofline.traffic)
#  2. smoke, then the default bench -> $OUT/bench.json
#  3. the kernel-trace profile of a short bench with its per-level split (prof.sh)
#  4. the SQ occupancy / stall pass (pmc_sq.sh)
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
ROUND=${ROUND:-r04}
export OUT=${OUT:-out}; mkdir -p $OUT
bash tools/gpu/pmc.sh || exit 1
python3 tools/pmc_summarize.py $OUT profiles/${ROUND}_level0_spmv_pmc.json "${COMMIT:-unknown}" > /dev/null || exit 1
cp profiles/${ROUND}_level0_spmv_pmc.json $OUT/level0_spmv_pmc.json
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
echo smoke-ok
timeout -k 10 900 python -u bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
head -c 400 $OUT/bench.json; echo
bash tools/gpu/prof.sh > $OUT/prof.out 2>&1 || { tail -20 $OUT/prof.out; exit 1; }
tail -16 $OUT/prof_levels.txt
bash tools/gpu/pmc_sq.sh > $OUT/pmc_sq.out 2>&1 || { tail -20 $OUT/pmc_sq.out; exit 1; }
head -20 $OUT/kernels_sq_pmc.txt
