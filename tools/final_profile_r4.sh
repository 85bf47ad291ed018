#!/bin/bash
# Evidence for profiles/ (round 4), all on ONE box in ONE call:
#  (1) FETCH / WRITE calibration, (2) rocprofv3 --kernel-trace --stats of bench.py's main leg (K1 + k_verify_seeds + k_sparse_frame),
#  (3) FETCH_SIZE / WRITE_SIZE of the chain's kernels for the L8 / RGB8 / L16 / 4K / noise workloads (separate --pmc passes) and
#  profiles/k1_traffic.json from them, (4) stage times of k_sparse_frame's workgroups and its flood phases, (5) kernel trace of the
#  pass with three batches in flight, (6) the full bench line, (7) kernel resources.
# usage: tools/final_profile_r4.sh <tag>        (on the GPU box, from the repo root)
TAG=$1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=gpurun_out/final_$TAG; mkdir -p $OUT; rm -f $OUT/*.txt
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d /tmp/calib_$C -- tools/ubench/fetch_calib > /dev/null 2>&1
  python3 - /tmp/calib_$C $C >> $OUT/calibration.txt <<'PY'
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True)[0]
agg = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    if r["Counter_Name"] == sys.argv[2]: agg[r["Kernel_Name"].split("(")[0]].append(float(r["Counter_Value"]))
for k, v in agg.items(): print("%-12s %-10s mean %.1f KB per launch of 1048576 KB moved  -> factor %.4f" % (sys.argv[2], k, sum(v)/len(v), sum(v)/len(v)/1048576.0))
PY
done
cat $OUT/calibration.txt
COMMON="--no-cpu-baseline --extra-pipeline 0 --no-extra --no-verify"
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/stats_$TAG -- python3 bench.py --steps 50 --warmup 3 $COMMON > $OUT/bench_under_rocprof.json 2> /dev/null
S=$(find /tmp/stats_$TAG -name "*kernel_stats.csv" | head -1); (head -1 $S; grep "agx::" $S) > $OUT/kernel_stats.csv; cut -c1-130 $OUT/kernel_stats.csv
echo "== pmc traffic"
: > $OUT/pmc_traffic.txt
for CFG in "256 1280 800 L8 0" "256 1280 800 RGB8 0" "256 1280 800 L16 0" "32 3840 2160 L8 0" "64 1280 800 L8 1"; do
  set -- $CFG
  for C in FETCH_SIZE WRITE_SIZE; do
    D=/tmp/pmc_${TAG}_$C; rm -rf $D
    FRAMES=$1 WIDTH=$2 HEIGHT=$3 FORMAT=$4 NOISE=$5 UNIQUE=$([ $2 = 3840 ] && echo 8 || echo 64) rocprofv3 --kernel-trace --pmc $C --output-format csv -d $D -- python3 tools/sweep.py 0 > /dev/null 2>&1
    python3 - $D $C "$1x$2x$3_$4$([ $5 = 1 ] && echo _noise)" >> $OUT/pmc_traffic.txt <<'PY'
import csv, glob, sys, collections
agg = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "agx::" in r["Kernel_Name"] and r["Counter_Name"] == sys.argv[2]:
            agg[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
for k, v in agg.items():
    v = v[len(v)//2:]
    print("%s %s %s mean %.6g KB (n=%d)" % (sys.argv[3], k, sys.argv[2], sum(v)/len(v), len(v)))
PY
    rm -rf $D
  done
done
cat $OUT/pmc_traffic.txt
python3 - $OUT/pmc_traffic.txt $TAG > $OUT/k1_traffic.json <<'PY'
import json, sys, collections, re
# bytes per K1 launch = FETCH_SIZE (KB; 64-byte requests: x2 for K1's 128-byte streaming reads, per the calibration) + WRITE_SIZE (KB)
d = collections.defaultdict(dict)
for line in open(sys.argv[1]):
    m = re.match(r"(\S+) (agx::\S+?(?:<[^>]*>)?) (FETCH_SIZE|WRITE_SIZE) mean (\S+) KB", line)
    if m and "k_blur_hessian" in m.group(2): d[m.group(1)][m.group(3)] = float(m.group(4))
out = {}
for cfg, c in d.items():
    if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
        out[cfg] = {"bytes_per_launch": (2 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0,
                    "source": "profiles/r4_%s_pmc_traffic.txt (FETCH_SIZE x2 for streaming reads per profiles/r4_%s_calibration.txt, + WRITE_SIZE); a PMC pass of its own on another run -- not a counter of the bench run that quotes it" % (sys.argv[2], sys.argv[2])}
print(json.dumps(out, indent=1))
PY
cat $OUT/k1_traffic.json
echo "== k_sparse_frame stages"
python3 tools/sparse_frame_phases.py 2>/dev/null > $OUT/sparse_frame_phases.txt; cat $OUT/sparse_frame_phases.txt
FUSED=1 python3 tools/flood_phases.py 2>/dev/null > $OUT/flood_phases_sparse_frame.txt; cat $OUT/flood_phases_sparse_frame.txt
echo "== three batches in flight"
D=/tmp/pipe_$TAG; rm -rf $D
rocprofv3 --kernel-trace --output-format csv -d $D -- python3 bench.py --steps 40 --warmup 3 --pipeline 3 $COMMON > $OUT/bench_pipeline3_under_rocprof.json 2> /dev/null
python3 - $D > $OUT/pipeline3_overlap.txt <<'PY'
import csv, glob, sys, statistics, collections
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "agx::" in r["Kernel_Name"]]
name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("agx::", "").split("<")[0]
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name(r)) for r in rows)
ev = ev[len(ev) // 3:]  # steady state
t0, t1 = ev[0][0], max(e[1] for e in ev)
dur = collections.defaultdict(list)
for s, e, n in ev: dur[n].append((e - s) / 1e3)
print("kernels of the pass with three batches in flight (rocprofv3 --kernel-trace), steady state, %d launches" % len(ev))
for n, v in dur.items(): print("  %-18s median %.1f us (min %.1f, max %.1f)" % (n, statistics.median(v), min(v), max(v)))
pts = sorted(set([s for s, e, n in ev] + [e for s, e, n in ev]))
k1 = sp = both = none = 0
for a, b in zip(pts[:-1], pts[1:]):
    m = (a + b) // 2
    has1 = any(s <= m < e and n == "k_blur_hessian" for s, e, n in ev)
    hass = any(s <= m < e and n != "k_blur_hessian" for s, e, n in ev)
    d = b - a
    if has1 and hass: both += d
    elif has1: k1 += d
    elif hass: sp += d
    else: none += d
tot = (t1 - t0)
print("  wall %.1f us: blur kernel alone %.1f %%, blur + a sparse kernel %.1f %%, sparse kernels alone %.1f %%, nothing %.1f %%" % (tot / 1e3, 100 * k1 / tot, 100 * both / tot, 100 * sp / tot, 100 * none / tot))
n1 = len(dur["k_blur_hessian"])
print("  per batch: %.1f us of wall time (%d batches)" % (tot / 1e3 / n1, n1))
PY
cat $OUT/pipeline3_overlap.txt
rm -rf $D
python3 bench.py --steps 50 --warmup 3 --full > $OUT/bench.json 2>/dev/null; cut -c1-300 $OUT/bench.json
python3 tools/kernel_resources.py > $OUT/kernel_resources.txt 2>/dev/null
