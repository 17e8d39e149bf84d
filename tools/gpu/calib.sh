set -o pipefail
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $PWD/$OUT/calib -o run -- tools/pmc_calib > $OUT/calib.log 2>&1 || exit 1
echo calib-ok
