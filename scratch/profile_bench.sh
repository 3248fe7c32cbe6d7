#!/bin/bash
# usage (on the GPU box): scratch/profile_bench.sh <tag>  -> $OUT/prof_<tag>/ (rocpd db) + bench JSON line
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
cd /tmp; export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $OUT/prof_$1 -o $1 -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $OUT/prof_$1.log 2>&1
grep '^{"metric"' $OUT/prof_$1.log > $OUT/prof_$1.bench.json
tail -1 $OUT/prof_$1.bench.json | cut -c1-160
