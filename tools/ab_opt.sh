# A/B of library options (WSFRAME_AMD_OPTIONS), interleaved on one box:
#   bash tools/ab_opt.sh <tag> "<bench args>" "<opts>|<opts>|..." [rounds]
# Results go to $AB_OUT (default: ab_out/ in the current directory).
set -o pipefail
tag=$1; args=$2; IFS='|' read -ra OPTS <<< "$3"; rounds=${4:-3}
export AB_OUT=${AB_OUT:-ab_out}
mkdir -p "$AB_OUT"
for r in $(seq 1 $rounds); do
  for o in "${OPTS[@]}"; do
    WSFRAME_AMD_OPTIONS="$o" timeout -k 10 180 python bench.py $args --full --no-cpu --no-e2e --no-xor-stream > "$AB_OUT/ab_one.json" 2>/dev/null || { echo "FAIL $o"; exit 1; }
    python -c "
import json,os;d=json.load(open(os.path.join(os.environ['AB_OUT'], 'ab_one.json')));r=d['roofline']
print('$o', '$args', d['ms_per_step'], r['frac'], r.get('kernel_ms_mean'), d['verified'])" | tee -a "$AB_OUT/ab_$tag.log"
  done
done
