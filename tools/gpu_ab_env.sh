#!/bin/bash
# A/B of environment settings (same library) on one bench configuration, same box.
# usage (GPU box, repo root): bash tools/gpu_ab_env.sh <config> <name>=<VAR=val[,VAR=val]> ...  ("base" = no change)
#   -> $OUT_DIR/ab/<config>_env_<name>.json (OUT_DIR: where the results go, default bench_out)
set -u
c=$1; shift
out=${OUT_DIR:-bench_out}/ab
mkdir -p "$out"
for spec in "base=" "$@"; do
  name=${spec%%=*}; vars=${spec#*=}
  ( IFS=','; for kv in $vars; do [ -n "$kv" ] && export "$kv"; done
    timeout -k 10 200 python bench.py --full --config "$c" --steps 40 --warmup 2 --no-cpu --kp-reps 20 > "$out/${c}_env_$name.json" 2> "$out/${c}_env_$name.err" ) || exit $?
  python3 -c "import json;b=json.loads(open('$out/${c}_env_$name.json').read().strip().splitlines()[-1]);print('$c $name',round(b['value'],1),round(b['roofline']['launch_ms'],4),round(b['kp_ms'],4))"
done
