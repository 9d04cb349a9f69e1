#!/bin/bash
# same-box solo times (us) per (kind, tag) under environment settings, for kinds matching a prefix: bash tools/ab_tags.sh "<kind prefix>" "<VAR=val>" ...
pre="$1"; shift
export OUT=${OUT:-bench_out}    # output folder
mkdir -p $OUT
for cfg in "$@"; do
  rm -f $OUT/map.json    # (a failed run must not leave the previous configuration's table to be read)
  env $cfg BENCH_LAUNCH_MAP=$OUT/map.json python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
  python - "$pre" "$cfg" <<'PY'
import os, json, sys, collections
m = json.load(open(os.environ["OUT"] + "/map.json"))
agg = collections.OrderedDict()
for e in m:
    if e["kind"].startswith(sys.argv[1]):
        k = (e["kind"], e["tag"], tuple(e["kernels"][:1]))
        agg.setdefault(k, []).append(e["ms"])
for (kind, tag, kern), v in agg.items():
    print(f"[{sys.argv[2]}] {kind} {tag} n={len(v)} avg {sum(v)/len(v)*1e3:.1f} us {kern}")
PY
done
