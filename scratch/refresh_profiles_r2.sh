#!/bin/bash
# usage (GPU box): scratch/refresh_profiles_r2.sh -> $OUT/r02/: kernel-trace stats of the bench command, FETCH/WRITE PMC passes, LDS / issue counters
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
R=$GRAFT_REPO_ROOT
cd $R; mkdir -p $OUT/r02
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/r02/trace -o r02 -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $OUT/r02/trace.log 2>&1
grep '^{"metric"' $OUT/r02/trace.log | tail -1 > $OUT/r02/trace_bench_line.json
f=$(ls $OUT/r02/trace/*.db 2>/dev/null | head -1); [ -z "$f" ] && f=$(ls $OUT/r02/trace/*/*.db | head -1)
python $R/scratch/rocpd_stats.py $f 70 > $OUT/r02/kernel_stats.txt
rm -rf $OUT/r02/trace
for set in "FETCH_SIZE" "WRITE_SIZE"; do
  rocprofv3 --kernel-trace --pmc $set -d $OUT/r02/pmc_traffic -o $set --output-format csv -- python $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-graph > $OUT/r02/pmc_$set.log 2>&1
done
python $R/scratch/pmc_traffic.py $OUT/r02/pmc_traffic $OUT/r02/pmc_traffic.json > $OUT/r02/pmc_traffic_top.txt
i=0
for set in "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INSTS_SALU" \
           "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_COEXEC_CYCLES SQ_INSTS_VALU_TRANS_F32"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --pmc $set -d $OUT/r02/pmc_sq -o p$i --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-graph > $OUT/r02/pmc_sq$i.log 2>&1
done
python - <<PY > $OUT/r02/pmc_sq.txt
import csv, glob, collections, re
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/r02/pmc_sq/*counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        k = re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"]).split("(")[0][:70]
        if any(x in k for x in ("gemm", "conv_halo", "attn_")):
            agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
print("# rocprofv3 --pmc (two passes) over bench.py --no-graph: per-dispatch averages of the MFMA kernels")
for k, c in sorted(agg.items(), key=lambda kv: -sum(kv[1].get("SQ_WAVE_CYCLES", [0]))):
    n = len(next(iter(c.values())))
    print(f"{k}  (x{n})")
    for name, v in sorted(c.items()): print(f"   {name:30s} {sum(v)/len(v):16.0f}")
    if "SQ_VALU_MFMA_BUSY_CYCLES" in c and "SQ_WAVE_CYCLES" in c: pass
PY
rm -rf $OUT/r02/pmc_sq $OUT/r02/pmc_traffic
ls -la $OUT/r02
