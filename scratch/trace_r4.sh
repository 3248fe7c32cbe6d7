#!/bin/bash
# usage (GPU box): scratch/trace_r4.sh [tag] -> $OUT/<tag>/: bench line, kernel-trace stats and one-replay timeline of bench.py
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
TAG=${1:-r04}
R=$GRAFT_REPO_ROOT
cd $R; mkdir -p $OUT/$TAG
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/$TAG/trace -o $TAG -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $OUT/$TAG/trace.log 2>&1
grep '^{"metric"' $OUT/$TAG/trace.log | tail -1 > $OUT/$TAG/trace_bench_line.json
f=$(ls $OUT/$TAG/trace/*.db 2>/dev/null | head -1); [ -z "$f" ] && f=$(ls $OUT/$TAG/trace/*/*.db | head -1)
python $R/scratch/rocpd_stats.py $f 80 > $OUT/$TAG/kernel_stats.txt
python $R/scratch/step_timeline.py $f $OUT/$TAG/step_timeline.txt
rm -rf $OUT/$TAG/trace
ls -la $OUT/$TAG
