#!/bin/bash
# same-box solo times (us) of launch kinds under environment settings: bash tools/ab_kinds.sh "<kind,kind>" "<VAR=val>" ...
kinds="$1"; shift
export OUT=${OUT:-bench_out}    # output folder
mkdir -p $OUT
for cfg in "$@"; do
  rm -f $OUT/map.json    # (a failed run must not leave the previous configuration's table to be read)
  env $cfg BENCH_LAUNCH_MAP=$OUT/map.json python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > /dev/null 2>&1
  python - "$kinds" "$cfg" <<'PY'
import os, json, sys
m = json.load(open(os.environ["OUT"] + "/map.json"))
for k in sys.argv[1].split(","):
    r = [e["ms"] for e in m if e["kind"] == k]
    print(f"[{sys.argv[2]}] {k}: n={len(r)} total {sum(r)*1e3:.1f} us")
print(f"[{sys.argv[2]}] solo step {sum(e['ms'] for e in m):.3f} ms")
PY
done
