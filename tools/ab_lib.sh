# A/B of builds of libwsframe_amd.so, interleaved on one box:
#   bash tools/ab_lib.sh <tag> "<bench args>|<bench args>|..." [rounds] [libs]
# libs: space-separated names; "new" = util_amd/libwsframe_amd.so, X = util_amd/libwsframe_amd_X.so
# (default "base new"). Results go to $AB_OUT (default: ab_out/ in the current directory).
set -o pipefail
tag=$1; IFS='|' read -ra CASES <<< "$2"; rounds=${3:-3}; libs=${4:-base new}
export AB_OUT=${AB_OUT:-ab_out}
mkdir -p "$AB_OUT"
for r in $(seq 1 $rounds); do
  for lib in $libs; do
    for c in "${CASES[@]}"; do
      if [ $lib = new ]; then unset WSFRAME_AMD_LIB; else export WSFRAME_AMD_LIB=$PWD/util_amd/libwsframe_amd_$lib.so; fi
      timeout -k 10 180 python bench.py $c --full --no-cpu --no-e2e --no-xor-stream > "$AB_OUT/ab_one.json" 2>/dev/null || { echo "FAIL $lib $c"; exit 1; }
      python -c "
import json,os,sys;d=json.load(open(os.path.join(os.environ['AB_OUT'], 'ab_one.json')));r=d['roofline']
print('$lib', '$c'.strip(), d['ms_per_step'], r['frac'], r.get('kernel_ms_mean'), d['verified'])" | tee -a "$AB_OUT/ab_$tag.log"
    done
  done
done
