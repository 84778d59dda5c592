#!/bin/bash
# usage: ov_sweep.sh <label> <bench args...>   (--full: the secondary leg is reported beside the headline one)
L=$1; shift
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
for o in 8 4 3 5 8 4 3 5; do
  timeout -k 10 200 python bench.py --full --cpu-seconds 0 --no-parity --no-cfg5 --no-api --overlap $o "$@" > "$T/ovs.json" 2> "$T/ovs.err" || { echo FAILED; tail -n 3 "$T/ovs.err"; exit 1; }
  python - "$L" $o "$T/ovs.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[3]))
s="%s overlap %s: %s %.3f M traj/s %.2f ms frac %.4f" % (sys.argv[1], sys.argv[2], d["dtype"], d["value"]/1e6, d["ms_per_step"], d["roofline"]["frac"])
for k in ("f32","f64_fast"):
    if k in d and isinstance(d[k],dict) and "value" in d[k]: s+=" | %s %.3f M %.2f ms" % (k, d[k]["value"]/1e6, d[k]["ms_per_step"])
print(s, flush=True)
PY
done
