#!/bin/bash
# tuning only: bench each build_variants/lib_<name>.so given on the command line (run on the GPU box)
out=${BENCH_OUT:-bench_out}
mkdir -p "$out"
for v in "$@"; do
  NEB_LIB_PATH=$PWD/build_variants/lib_$v.so timeout -k 10 120 python bench.py --full --cpu-frames 0 > "$out/ab_$v.json" 2> "$out/ab_$v.err" || exit 1
  python - "$v" "$out" <<'PY'
import json, sys
d = json.load(open(f"{sys.argv[2]}/ab_{sys.argv[1]}.json"))
print(sys.argv[1], round(d["value"], 1), "fps  gi_us", round(d["kernel_us"]["gi_trace"], 1))
PY
done
