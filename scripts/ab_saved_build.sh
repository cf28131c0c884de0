#!/bin/bash
# A/B of a SAVED build of the parent commit against the library of the working tree, run from the same tree on one box
# (the protocol of profiles/lin_uniform_ab.txt and profiles/uniform_records_ab.txt):
#   scripts/ab_saved_build.sh <parent libtumnmpc.so> [headline] [trace] [full] | [headline1] [ktrace] [ktrace3] [onestream] [dump] [fullbench]
#     headline  python bench.py, six fresh processes each, interleaved parent / change (headline1: the same with --streams 1)
#     trace     rocprofv3 --kernel-trace --stats -- python bench.py --streams 1 (kernel trace only, no counters) for each build: average and
#               standard deviation per kernel; then bench.py --full --no-other-configs --no-cpu-baseline for each (value_single_stream)
#     full      bench.py --dump-outputs (--steps 20 --warmup 3) for each build and the bitwise comparison of every .npy, then bench.py --full
#     ktrace, onestream | dump, fullbench: the two halves of trace | of full on their own
#     ktrace3   the kernel trace of the DEFAULT run (three streams) for each build: kernels that wait for room beside the other capsules' kernels
# The parent's library is built by the same compiler from `git archive <parent>` with the command line of __graft_entry__.build() and
# loaded through TUM_NMPC_LIB. Every process runs under its own timeout; the chain stops at the first non-zero exit.
# Results under $AB_OUT (default: ab_out/, which git ignores).
set -u
PARENT=$(readlink -f "$1"); shift
LEGS="${*:-headline trace full}"
OUT=${AB_OUT:-ab_out}; mkdir -p $OUT
export TMPDIR=/tmp
use() { if [ "$1" = parent ]; then export TUM_NMPC_LIB=$PARENT; else unset TUM_NMPC_LIB; fi; }
die() { echo "$1 rc=$2"; exit "$2"; }
EXP=""
for leg in $LEGS; do case $leg in trace) EXP="$EXP ktrace onestream" ;; full) EXP="$EXP dump fullbench" ;; *) EXP="$EXP $leg" ;; esac; done
for leg in $EXP; do
case $leg in
headline|headline1)
  # headline1: the same six pairs on ONE stream (bench.py --streams 1)
  if [ $leg = headline1 ]; then HL_ARGS="--streams 1"; HL=s1_; else HL_ARGS=""; HL=""; fi
  for i in 1 2 3 4 5 6; do for w in parent change; do
    use $w
    timeout -k 10 240 python bench.py $HL_ARGS > $OUT/${HL}${w}_$i.out 2> $OUT/${HL}${w}_$i.err < /dev/null || die "$leg $w $i" $?
    grep metric $OUT/${HL}${w}_$i.out > $OUT/${HL}${w}_$i.json
    python -c "import json; d = json.load(open('$OUT/${HL}${w}_$i.json')); print('$leg', '$w', $i, 'value', round(d['value']), 'ms/step', round(d['ms_per_step'], 4))"
  done; done ;;
ktrace|ktrace3)
  # ktrace: one stream; ktrace3: the default run's three streams (what a kernel waits for beside the other capsules' kernels shows here only)
  if [ $leg = ktrace3 ]; then TR_ARGS=""; TR=trace3; else TR_ARGS="--streams 1"; TR=trace; fi
  for w in parent change; do
    use $w
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_$w -o s -- python bench.py $TR_ARGS --no-cpu-baseline \
        --no-schedule-legs --no-other-configs --steps 20 --warmup 3 > $OUT/${TR}_$w.log 2>&1 < /dev/null || die "$TR $w" $?
    python - $OUT/stats_$w > $OUT/kernel_avg_std_${TR}_$w.txt <<'EOF' || die "$TR summary $w" $?
import collections, csv, glob, statistics, sys
d = collections.defaultdict(list)
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        d[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for k, v in sorted(d.items(), key=lambda kv: -sum(kv[1])):
    if any(s in k for s in ("lin_", "cond_", "ipm_", "expand_", "lpt_", "cold_start")):
        print("%-64s n %3d  avg %9.0f ns  std %8.0f  min %9d  max %9d" % (k[:64], len(v), statistics.mean(v), statistics.pstdev(v), min(v), max(v)))
EOF
    rm -rf $OUT/stats_$w
    echo "$w: $TR, traced value $(grep metric $OUT/${TR}_$w.log | python -c "import json, sys; print(round(json.loads(sys.stdin.read())['value']))")"; cat $OUT/kernel_avg_std_${TR}_$w.txt
  done ;;
onestream)
  for w in parent change; do
    use $w
    timeout -k 10 420 python bench.py --full --no-other-configs --no-cpu-baseline > $OUT/full1_$w.out 2> $OUT/full1_$w.err < /dev/null || die "one-stream leg $w" $?
    grep metric $OUT/full1_$w.out > $OUT/full1_$w.json
    python -c "import json; d = json.load(open('$OUT/full1_$w.json')); print('$w', {k: round(v) for k, v in d.items() if k.startswith('value')})"
  done ;;
dump)
  for w in parent change; do
    use $w
    rm -rf /tmp/ab_dump_$w
    timeout -k 10 240 python bench.py --dump-outputs /tmp/ab_dump_$w --steps 20 --warmup 3 --no-cpu-baseline > $OUT/dump_$w.out 2> $OUT/dump_$w.err < /dev/null || die "dump $w" $?
  done
  python - /tmp/ab_dump_parent /tmp/ab_dump_change <<'EOF' | tee $OUT/dump_compare.txt
import os, sys
import numpy as np
a, b = sys.argv[1:3]
fa, fb = (sorted(f for f in os.listdir(d) if f.endswith(".npy")) for d in (a, b))
assert fa == fb and fa, (fa, fb)
bad = 0
for f in fa:
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    print(f, x.shape, x.dtype, "bit-identical" if same else "DIFFERENT")
    bad += not same
print("files", len(fa), "different", bad)
EOF
  ;;
fullbench)
  for w in parent change; do
    use $w
    timeout -k 10 600 python bench.py --full > $OUT/full_$w.out 2> $OUT/full_$w.err < /dev/null || die "full $w" $?
    grep metric $OUT/full_$w.out > $OUT/full_$w.json
  done ;;
esac
done
