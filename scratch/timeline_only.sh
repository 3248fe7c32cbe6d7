#!/bin/bash
# usage (GPU box): scratch/timeline_only.sh <tag>  -> $OUT/<tag>_timeline.txt (one replayed step, kernel by kernel)
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
R=$GRAFT_REPO_ROOT; T=${1:-tl}
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/tl_$T -o tl -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $OUT/${T}_trace.log 2>&1
f=$(ls /tmp/tl_$T/*.db 2>/dev/null | head -1); [ -z "$f" ] && f=$(ls /tmp/tl_$T/*/*.db | head -1)
python $R/scratch/step_timeline.py $f $OUT/${T}_timeline.txt
grep '^{"metric"' $OUT/${T}_trace.log | tail -1 | cut -c1-200
