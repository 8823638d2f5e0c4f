#!/bin/bash
# A/B/A/B... of bench.py between TWO BUILDS of libfgvc_hip.so on one box: the parent commit's library (built from a checkout of the parent,
# copied aside) against this tree's, the Python above them this tree's (a change to csrc/ alone).  _lib.py loads $FGVC_HIP_LIB when set.
#     bash tools/ab_parent_lib.sh build/parent/libfgvc_hip.so [runs per arm, default 6] [extra bench flags]   ->   $AB_OUT/ab_parent_lib.log (AB_OUT: default build/ab, not tracked)
# Every run under its own time limit; the first failure ends the script.
PARENT=$(readlink -f "${1:?libfgvc_hip.so of the parent commit}"); RUNS=${2:-6}; shift; shift
[ -f "$PARENT" ] || { echo "no such library: $PARENT"; exit 1; }
OUT=${AB_OUT:-build/ab}/ab_parent_lib.log; mkdir -p "$(dirname "$OUT")"; : > $OUT
ONE=$(dirname "$OUT")/ab_one          # one run's line and stderr, beside the log
for rep in $(seq $RUNS); do
  for arm in parent change; do
    if [ $arm = parent ]; then export FGVC_HIP_LIB=$PARENT; name="parent commit"; else unset FGVC_HIP_LIB; name="this change"; fi
    timeout -k 10 300 python3 bench.py --gpus 1 --steps 60 --warmup 10 "$@" > "$ONE.json" 2> "$ONE.err" || { echo "bench failed ($name)" >> $OUT; tail -3 "$ONE.err" >> $OUT; cat $OUT; exit 1; }
    python3 - "$name" "$ONE.json" >> $OUT <<'PY' || exit 1
import json, sys
d = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
print(f"{sys.argv[1]:22s} {d['value']:8.1f} frames/s  {d['ms_per_step']:.4f} ms/step")
PY
  done
done
unset FGVC_HIP_LIB
python3 - $OUT <<'PY'
import statistics, sys
arms = {}
for l in open(sys.argv[1]):
    f = l.split()
    if len(f) >= 6 and f[3] == "frames/s":
        arms.setdefault(f[0] + " " + f[1], []).append((float(f[2]), float(f[4])))
with open(sys.argv[1], "a") as out:
    for k, v in arms.items():
        fps, ms = [a for a, _ in v], [b for _, b in v]
        out.write(f"{k:22s} median {statistics.median(ms):.4f} ms/step (min {min(ms):.4f}, max {max(ms):.4f})  median {statistics.median(fps):.1f} frames/s "
                  f"(min {min(fps):.1f}, max {max(fps):.1f})  n={len(v)}\n")
    if len(arms) == 2:
        (a, va), (b, vb) = arms.items()
        lo_a, hi_a, lo_b, hi_b = min(m for _, m in va), max(m for _, m in va), min(m for _, m in vb), max(m for _, m in vb)
        out.write(f"ranges of ms/step: {a} [{lo_a:.4f}, {hi_a:.4f}], {b} [{lo_b:.4f}, {hi_b:.4f}]: {'disjoint' if hi_b < lo_a or hi_a < lo_b else 'OVERLAP'}\n")
PY
cat $OUT
