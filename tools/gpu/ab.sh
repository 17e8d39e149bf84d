# A/B of engine variants on the per-level kernel times of the bench workload (kernel-trace profile
# of a short bench per variant).  Variants: label=ENV=VAL[,ENV=VAL...] arguments, e.g.
#   bash tools/gpu/ab.sh head= prev=SSS_AMG_LIB=amg_amd/lib_ab/libsss_amg.so nodict=SSS_HIP_DICT=0
cd "$(dirname "$0")/../.." || exit 1
export OUT=${OUT:-out}; mkdir -p $OUT/ab
for v in "$@"; do
    label=${v%%=*}; envs=${v#*=}
    ( IFS=','; for kv in $envs; do [ -n "$kv" ] && export "$kv"; done
      [ -n "$SSS_AMG_LIB" ] && export SSS_AMG_LIB="$PWD/${SSS_AMG_LIB#$PWD/}"
      bash tools/gpu/prof.sh > $OUT/ab/$label.out 2>&1 ) || { echo "variant $label failed"; tail -20 $OUT/ab/$label.out; exit 1; }
    cp $OUT/prof_levels.txt $OUT/ab/levels_$label.txt
    cp $OUT/prof_bench.json $OUT/ab/bench_$label.json
    echo "== $label: $(grep -o '"ms_per_step": [0-9.]*' $OUT/ab/bench_$label.json)"
    tail -4 $OUT/ab/levels_$label.txt
done
rm -rf $OUT/prof_cur
