#!/bin/bash
# usage (GPU box): scratch/refresh_profiles_r4b.sh -> $OUT/r04/: the default 250-step bench line and the secondary bench lines of round 4
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
R=$GRAFT_REPO_ROOT
cd $R; mkdir -p $OUT/r04
python bench.py --full > $OUT/r04/default.log 2>&1; grep '^{"metric"' $OUT/r04/default.log | tail -1 > $OUT/r04/bench_default_run.json
python bench.py --full --precision bf16 --steps 100 --warmup 20 --no-cpu-baseline > $OUT/r04/bf16.log 2>&1; grep '^{"metric"' $OUT/r04/bf16.log | tail -1 > $OUT/r04/bench_bf16.json
TB_FORCE_DIST=1 python bench.py --steps 100 --warmup 20 --no-cpu-baseline --no-roofline > $OUT/r04/dist1.log 2>&1; grep '^{"metric"' $OUT/r04/dist1.log | tail -1 > $OUT/r04/bench_force_dist_one_rank.json
python bench.py --full --vae --steps 60 --warmup 10 --no-cpu-baseline > $OUT/r04/vae.log 2>&1; grep '^{"metric"' $OUT/r04/vae.log | tail -1 > $OUT/r04/bench_with_vae_encoder.json
python bench.py --full --batch 16 --steps 60 --warmup 10 --no-cpu-baseline > $OUT/r04/b16.log 2>&1; grep '^{"metric"' $OUT/r04/b16.log | tail -1 > $OUT/r04/bench_config5_batch16.json
python bench.py --full --workload sd21 --steps 40 --warmup 10 --no-cpu-baseline > $OUT/r04/sd21.log 2>&1; grep '^{"metric"' $OUT/r04/sd21.log | tail -1 > $OUT/r04/bench_config4_sd21_96.json
python bench.py --full --precision fp32 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/r04/fp32.log 2>&1; grep '^{"metric"' $OUT/r04/fp32.log | tail -1 > $OUT/r04/bench_fp32_mode.json
for f in $OUT/r04/bench_*.json; do echo $f; cut -c1-160 $f; done
