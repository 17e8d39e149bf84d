# A/B of per-level kernel times: the default, then each "VAR=value" given in $AB (space-separated)
cd "$(dirname "$0")/../.." || exit 1
export TMPDIR=/tmp
export OUT=${OUT:-out}; mkdir -p $OUT/ab
bash tools/gpu/prof.sh > $OUT/ab/base.out 2>&1 || { tail -20 $OUT/ab/base.out; exit 1; }
cp $OUT/prof_levels.txt $OUT/ab/base_levels.txt
cp $OUT/prof_bench.json $OUT/ab/base_bench.json
echo "== base"; cat $OUT/ab/base_levels.txt
python3 -c "import json,sys; r=json.load(open(sys.argv[1]))['roofline']; print('roofline ms', r['avg_launch_ms'], 'cycle_storage ms', r['cycle_storage']['avg_launch_ms'])" $OUT/ab/base_bench.json
for kv in $AB; do
  t=$(echo "$kv" | tr "/" "_")
  env "$kv" bash tools/gpu/prof.sh > "$OUT/ab/$t.out" 2>&1 || { tail -20 "$OUT/ab/$t.out"; exit 1; }
  cp $OUT/prof_levels.txt "$OUT/ab/${t}_levels.txt"
  cp $OUT/prof_bench.json "$OUT/ab/${t}_bench.json"
  echo "== $kv"; cat "$OUT/ab/${t}_levels.txt"
  python3 -c "import json,sys; r=json.load(open(sys.argv[1]))['roofline']; print('roofline ms', r['avg_launch_ms'], 'cycle_storage ms', r['cycle_storage']['avg_launch_ms'])" "$OUT/ab/${t}_bench.json"
done
