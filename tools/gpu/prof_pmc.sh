# kernel-trace profile + per-level breakdown (prof.sh), then the level-0 PMC passes (pmc.sh),
# summarised into $OUT/level0_spmv_pmc.json
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
bash tools/gpu/prof.sh || exit 1
bash tools/gpu/pmc.sh || exit 1
python3 tools/pmc_summarize.py $OUT $OUT/level0_spmv_pmc.json
