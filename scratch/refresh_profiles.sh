#!/bin/bash
# usage (GPU box): scratch/refresh_profiles.sh  -> default bench run, rocprofv3 kernel stats of the same command, FETCH/WRITE PMC passes
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
R=$GRAFT_REPO_ROOT
cd $R
python bench.py --full > $OUT/bench_default.log 2>&1
grep '^{"metric"' $OUT/bench_default.log | tail -1 > $OUT/bench_default.json
cp $OUT/bench_kernel_table.json $OUT/bench_default_kernel_table.json
scratch/profile_bench.sh r01final
scratch/pmc_bench.sh > /dev/null 2>&1
tail -1 $OUT/bench_default.json | cut -c1-400
