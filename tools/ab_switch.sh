#!/bin/bash
# A/B/A/B... of one class switch of the encoder on one box, bench.py untouched: each run sets ResNet.<switch> and then runs bench.py as __main__
#     bash tools/ab_switch.sh fuse_s2_projection [runs per arm, default 6] [extra bench flags]   ->   $AB_OUT/ab_switch.log (AB_OUT: default build/ab, not tracked)
SW=${1:?switch name}; RUNS=${2:-6}; shift; shift
OUT=${AB_OUT:-build/ab}/ab_switch.log; mkdir -p "$(dirname "$OUT")"; : > $OUT
ONE=$(dirname "$OUT")/ab_one          # one run's line and stderr, beside the log
for rep in $(seq $RUNS); do
  for val in True False; do
    timeout -k 10 300 python3 -c "
import runpy, sys
from fgvc_amd.mmpt_api.backbones import ResNet
assert hasattr(ResNet, '$SW'), '$SW'
ResNet.$SW = $val
sys.argv = ['bench.py'] + sys.argv[1:]
runpy.run_path('bench.py', run_name='__main__')" --gpus 1 --steps 60 --warmup 10 "$@" > "$ONE.json" 2> "$ONE.err" || { echo "bench failed ($SW=$val)" >> $OUT; tail -3 "$ONE.err" >> $OUT; exit 1; }
    python3 - "$SW=$val" "$ONE.json" >> $OUT <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
print(f"{sys.argv[1]:32s} {d['value']:8.1f} frames/s  {d['ms_per_step']:.4f} ms/step")
PY
  done
done
python3 - $OUT <<'PY'
import statistics, sys
arms = {}
for l in open(sys.argv[1]):
    f = l.split()
    if len(f) >= 5 and f[2] == "frames/s":
        arms.setdefault(f[0], []).append((float(f[1]), float(f[3])))
with open(sys.argv[1], "a") as out:
    for k, v in arms.items():
        fps, ms = [a for a, _ in v], [b for _, b in v]
        out.write(f"{k:32s} median {statistics.median(ms):.4f} ms/step (min {min(ms):.4f}, max {max(ms):.4f})  median {statistics.median(fps):.1f} frames/s "
                  f"(min {min(fps):.1f}, max {max(fps):.1f})  n={len(v)}\n")
PY
cat $OUT
