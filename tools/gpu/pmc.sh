set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT
for c in FETCH_SIZE WRITE_SIZE; do
timeout -k 10 400 rocprofv3 --pmc $c --output-format csv -d $PWD/$OUT/pmc_$c -o run -- python3 tools/pmc_level0.py 400 5 > $OUT/pmc_$c.log 2>&1 || exit 1
echo pmc-$c-ok
done
