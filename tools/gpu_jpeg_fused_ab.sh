#!/bin/bash
# The fused JPEG transform against the unfused one: tools/jpeg_fused_ab.py's A/B (both forms alternating in one process), then one
# `rocprofv3 --kernel-trace --stats` run of each form for the kernels' own times. Writes OUTDIR/jpeg_fused_ab.txt, which is
# kept as profiles/jpeg_fused_ab.txt (the logs and traces stay in OUTDIR). Every step has its own time limit and the script ends at
# the first step that fails.
# usage: bash tools/gpu_jpeg_fused_ab.sh [OUTDIR, default /tmp/jpeg_fused_ab]
cd "$(dirname "$0")/.." || exit 1; export TMPDIR=/tmp
dir=${1:-/tmp/jpeg_fused_ab}; mkdir -p "$dir" || exit 1
out=$dir/jpeg_fused_ab.txt; cache=/tmp/jpeg_fused_ab_cache
summarise() {   # $1 = rocprof directory, $2 = label
  python3 - "$1" "$2" >> $out <<'PY'
import csv, glob, os, re, sys
f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1]
by = {}
for r in csv.DictReader(open(f)):
    m = re.search(r"(jpeg_\w+_kernel|resize_\w_kernel)", r["Kernel_Name"])
    if m:
        by.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(f"# {sys.argv[2]}: kernel, launches, median us, min us, max us")
for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    v = sorted(v)
    print(f"{k:28s} {len(v):4d} {v[len(v) // 2]:10.1f} {v[0]:10.1f} {v[-1]:10.1f}")
PY
}
timeout -k 10 420 python3 tools/jpeg_fused_ab.py --cache $cache --out $out > $dir/jpeg_fused_ab.log 2>&1 || { tail -20 $dir/jpeg_fused_ab.log; exit 1; }
echo "# The kernels' own times: one rocprofv3 --kernel-trace --stats run per form and file set (tools/jpeg_fused_ab.py --form F --reps 3:" >> $out
echo "# two warm-up runs, three timed ones and the whole call = 6 launches per kernel)" >> $out
for form in unfused fused; do
  for set in photos small; do
    if [ $set = photos ]; then sizes="--photos 435 --small 0"; label="435 files of 2000 x 1500"; else sizes="--photos 0 --small 870"; label="870 files of 224 x 224"; fi
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $dir/jpeg_fused_prof_${form}_$set -- \
      python3 tools/jpeg_fused_ab.py --form $form $sizes --reps 3 --cache $cache > $dir/jpeg_fused_prof_${form}_$set.log 2>&1 || { tail -20 $dir/jpeg_fused_prof_${form}_$set.log; exit 1; }
    summarise $dir/jpeg_fused_prof_${form}_$set "$form, $label"
  done
done
cat $out
