#!/bin/bash
# usage (GPU box): scratch/refresh_profiles_r3.sh -> $OUT/r03/: kernel-trace stats of the bench command, FETCH / WRITE PMC passes, SQ counters
OUT=${OUT:?set OUT to the absolute path of the directory that takes the results}
R=$GRAFT_REPO_ROOT
cd $R; mkdir -p $OUT/r03
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/r03/trace -o r03 -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline > $OUT/r03/trace.log 2>&1
grep '^{"metric"' $OUT/r03/trace.log | tail -1 > $OUT/r03/trace_bench_line.json
f=$(ls $OUT/r03/trace/*.db 2>/dev/null | head -1); [ -z "$f" ] && f=$(ls $OUT/r03/trace/*/*.db | head -1)
python $R/scratch/rocpd_stats.py $f 70 > $OUT/r03/kernel_stats.txt
rm -rf $OUT/r03/trace
for set in "FETCH_SIZE" "WRITE_SIZE"; do
  rocprofv3 --kernel-trace --pmc $set -d $OUT/r03/pmc_traffic -o $set --output-format csv -- python $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-graph > $OUT/r03/pmc_$set.log 2>&1
done
python $R/scratch/pmc_traffic.py $OUT/r03/pmc_traffic $OUT/r03/pmc_traffic.json > $OUT/r03/pmc_traffic_top.txt
i=0
for set in "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INSTS_SALU" \
           "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_COEXEC_CYCLES SQ_INSTS_VALU_TRANS_F32"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --pmc $set -d $OUT/r03/pmc_sq -o p$i --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-graph > $OUT/r03/pmc_sq$i.log 2>&1
done
python - <<PY > $OUT/r03/pmc_sq.txt
import csv, glob, collections, re
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("$OUT/r03/pmc_sq/*counter_collection.csv"):
    for r in csv.DictReader(open(f)):
        k = re.sub(r"\(anonymous namespace\)::|^void ", "", r["Kernel_Name"]).split("(")[0][:70]
        if any(x in k for x in ("gemm", "conv_halo", "attn_")):
            grid = r.get("Grid_Size", "")
            if k.startswith("attn_") and "_il_" in k: k = k + " grid=" + grid   # the L0 self-attention launches have their own symbols
            agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
print("# rocprofv3 --pmc (two passes) over bench.py --no-graph: per-dispatch averages of the MFMA kernels")
for k, c in sorted(agg.items(), key=lambda kv: -sum(kv[1].get("SQ_WAVE_CYCLES", [0]))):
    n = len(next(iter(c.values())))
    print(f"{k}  (x{n})")
    for name, v in sorted(c.items()): print(f"   {name:30s} {sum(v)/len(v):16.0f}")
PY
python $R/scratch/mfma_busy.py $OUT/r03/pmc_sq.txt $OUT/r03/mfma_busy.json > $OUT/r03/mfma_busy.txt
rm -rf $OUT/r03/pmc_sq $OUT/r03/pmc_traffic
ls -la $OUT/r03
