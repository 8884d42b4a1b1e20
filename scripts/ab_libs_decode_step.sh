#!/bin/bash
# A/B of the whole graph-captured decode step between library builds, same box, interleaved twice:
#   scripts/ab_libs_decode_step.sh OUTFILE "fp8:8 bf16:4 ..." libA.so libB.so ...
# Every run has its own time limit; the first run that fails, faults or times out ends the script with its status (nothing more
# is started on the GPU behind it) -- OUTFILE.log keeps the whole output of the runs so far.
set -o pipefail
OUT=$PWD/gpurun_out; mkdir -p $OUT
[ -d "$OUT" ] || exit 1
F=$OUT/$1; shift
CFGS=$1; shift
: > $F; : > $F.log
for rep in 1 2; do
  for lib in "$@"; do
    SRGPT_LIB=$lib timeout -k 10 600 python scripts/ubench_decode_step.py $CFGS 2>&1 | tee -a $F.log | grep "ms/step" | sed -E "s/ \{[^}]*\}//" >> $F
    st=("${PIPESTATUS[@]}")
    rc=${st[0]}                                 # the benchmark's own status (124 / 137: its time limit) ...
    [ $rc -eq 0 ] && [ ${st[2]} -ne 0 ] && rc=1  # ... or a run that printed no "ms/step" line
    if [ $rc -ne 0 ]; then
      echo "ab_libs_decode_step: $lib (rep $rep) ended with status $rc; stopping" >&2
      tail -n 20 $F.log >&2
      exit $rc
    fi
  done
done
cat $F
