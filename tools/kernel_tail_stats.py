"""tuning only: mean / sd / min / max of the LAST N launches of the GI kernels in a rocprofv3 kernel trace (the *_kernel_stats.csv beside it
averages every launch, warm-up included).
usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py ... ; python tools/kernel_tail_stats.py DIR <label> [N = 19]"""
import collections
import csv
import glob
import statistics as st
import sys

d, label = sys.argv[1], sys.argv[2]
n = int(sys.argv[3]) if len(sys.argv) > 3 else 19
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
acc = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    acc[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
for k, v in sorted(acc.items()):
    if not any(s in k for s in ("gi_shade", "gi_raygen_trace", "gi_shadow_list")):
        continue
    v = [x[1] for x in sorted(v)][-n:]
    print(f"{label} {k.split('(')[0][:60]}: n {len(v)} mean {st.mean(v):.2f} sd {st.stdev(v):.2f} min {min(v):.2f} max {max(v):.2f} us")
