# What a convergence check costs on a context: the numbers of profiles/context_until.txt.
#   [OUT=results/context_until] bash tools/recipes/context_until.sh [SIZE=8192] [REPS=20] [CAP=80]
# 1. kernel times, profiler on, a run of its own: mean of the norm kernel and of every SOR kernel over the steady-state launches
# 2. end to end, profiler off: the until call against the plain solve at SIZE and at 2048
export TMPDIR=/tmp
SIZE=${1:-8192}; REPS=${2:-20}; CAP=${3:-80}
O=${OUT:-results/context_until}; rm -rf $O; mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O -o t -- python3 tools/context_until_probe.py trace --size $SIZE --cap $CAP --reps $REPS > $O/trace.log 2> $O/trace.err || { echo "trace run failed"; tail -5 $O/trace.err; exit 1; }
cat $O/trace.log
python3 - $O $SIZE <<'PY'
import csv, glob, re, sys
o, size = sys.argv[1], int(sys.argv[2])
rows = list(csv.DictReader(open(glob.glob(o + "/**/*kernel_trace.csv", recursive=True)[0])))
by = {}
for r in rows:
    by.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for name, us in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    steady = us[len(us) // 4:]              # the first quarter of a kernel's launches is its warm-up
    mean = sum(steady) / len(steady)
    short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:110]
    line = "%-110s %5d launches, steady %4d: mean %9.1f us  min %9.1f  max %9.1f" % (short, len(us), len(steady), mean, min(steady), max(steady))
    if "update_norm" in name:
        line += "   = %.0f GB/s at 8 B/cell" % (8.0 * size * size / mean / 1e3)
    if "sor_fused" in name:
        line += "   = %.0f GB/s at 12 B/cell" % (12.0 * size * size / mean / 1e3)
    print(line)
PY
timeout -k 10 400 python3 tools/context_until_probe.py overhead --size $SIZE 2048 --cap $CAP --reps $REPS | tee $O/overhead.log
