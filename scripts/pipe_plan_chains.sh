#!/bin/bash
# The kernels every branch of plan_pipeline launches, a SAVED build of the parent commit against the library of the working tree:
#   scripts/pipe_plan_chains.sh <parent libtumnmpc.so> [report]
# scripts/pipe_plan_chains.py under `rocprofv3 --kernel-trace` (nothing else traced), once per library -- the parent's is loaded through
# TUM_NMPC_LIB, as scripts/ab_saved_build.sh does --, each run under its own timeout, the chain stops at the first non-zero exit. Then the
# comparison: ordered kernel names per capsule, and X, U, cost, status bit for bit. Scratch under $AB_OUT (default: ab_out/, which git ignores).
set -u -o pipefail
PARENT=$(readlink -f "$1"); REPORT=${2:-/dev/stdout}
OUT=${AB_OUT:-ab_out}/chains; rm -rf $OUT; mkdir -p $OUT
export TMPDIR=/tmp
one() {          # one <parent|change>
  if [ "$1" = parent ]; then export TUM_NMPC_LIB=$PARENT; else unset TUM_NMPC_LIB; fi
  timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d $OUT/trace_$1 -o t -- python scripts/pipe_plan_chains.py run $OUT/out_$1 \
      > $OUT/run_$1.log 2>&1 < /dev/null || { echo "run $1 rc=$?"; tail -20 $OUT/run_$1.log; return 1; }
}
one parent && one change && unset TUM_NMPC_LIB && \
  python scripts/pipe_plan_chains.py compare $OUT/out_parent $OUT/trace_parent $OUT/out_change $OUT/trace_change > $REPORT
