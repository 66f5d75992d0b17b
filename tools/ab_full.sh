#!/bin/bash
# like tools/ab.sh but also prints predict
read WL N B <<< "$1"; shift
T=$(mktemp); trap 'rm -f "$T"' EXIT
for L in "$@"; do
  NIMFM_HIP_LIB=$(pwd)/nimfm_amd/lib/$L python3 bench.py --workload $WL --n $N --batch $B --full --no-cpu-baseline > "$T"
  python3 - "$L" "$WL" "$T" <<'PY'
import json, sys
j = json.load(open(sys.argv[3])); r = j["roofline"]
print("%-22s %-9s %.4g samples/s frac %.4f %s predict %.4g (%.3f)" % (sys.argv[1], sys.argv[2], j["value"], r["frac"], {k: round(v * 1e3, 1) for k, v in r["avg_ms"].items() if v and k != "schedule"}, j["predict"]["value"], j["predict"]["roofline_frac"]))
PY
done
