#!/bin/bash
# Same-box A/B of library builds under gpurun_libs/ on the WHOLE bench line (other workloads, stage-A legs, drop-in legs):
#   bash tools/ab_full.sh "old F"   -> $OUT/ab_full_<name>.json (OUT defaults to /tmp/ab_full) + a one-line digest each
D=3dgs_hierarchical_training_amd/csrc
cp $D/libgsr_hip.so /tmp/cur.so
OUT=${OUT:-/tmp/ab_full}
mkdir -p $OUT
for w in $1; do
  cp gpurun_libs/lib_$w.so $D/libgsr_hip.so
  timeout 900 python bench.py --full --no-cpu-baseline > $OUT/ab_full_$w.json 2>/dev/null
  python - <<PY
import json
d = json.loads(open("$OUT/ab_full_$w.json").read().strip().splitlines()[-1])
ow = d.get("other_workloads", {})
print("$w", round(d["value"], 1), {k: (round(v.get("ms_per_step", v.get("image_iteration_ms", 0)), 4) if isinstance(v, dict) else v) for k, v in ow.items()},
      "dropin_autopatch", round(d.get("dropin_autopatch", {}).get("ms_per_step", 0), 4))
PY
done
cp /tmp/cur.so $D/libgsr_hip.so
