#!/bin/bash
# Store-side PMC passes for the pair-HMM kernel on the headline workload: vector store instructions, the write requests
# between the vector L1 and L2 and at L2, and the vector-memory busy / stall counters.  One rocprofv3 run per counter
# group, --kernel-trace only (as tools/pmc_pair.sh).  Run it for a full build and for its -DPAIR_EXP_STOP=3 build
# (DAFS_HIP_LIB=...): the difference is sweep 4's share.  A stop build computes no outputs, so the bench runs plain.
#   [DAFS_HIP_LIB=dafs_amd/_exp/libdafs_NAME.so] bash tools/pmc_pair_stores.sh <outdir>
# Prints one line per counter: the average per launch of k_pairhmm*.
set -e
out=${1:?usage: bash tools/pmc_pair_stores.sh <outdir>}
mkdir -p "$out"
root=$(pwd)
cd /tmp && export TMPDIR=/tmp
i=0
for grp in "SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_INST_CYCLES_VMEM_WR SQ_INST_CYCLES_VMEM_RD SQ_ACTIVE_INST_VMEM SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES" \
           "TCP_TCC_WRITE_REQ_sum TCP_PENDING_STALL_CYCLES_sum" \
           "TA_FLAT_WRITE_WAVEFRONTS_sum TA_BUSY_avr" \
           "TCC_WRITE_sum TCC_REQ_sum"; do  # two counters of a block per pass: eight TCP / TA counters in one exceed the hardware (error 38, and the run hangs)
  i=$((i+1))
  timeout -k 10 120 rocprofv3 --pmc $grp --kernel-trace --output-format csv -d "$root/$out/p$i" -o p -- python3 "$root/bench.py" --gpus 1 --steps 3 --warmup 1 $BENCH_FLAGS > "$root/$out/p$i.log" 2>&1 || { rc=$?; echo "group $i failed ($rc)"; if [ $rc -ge 124 ]; then exit $rc; fi; }
done
cd "$root"
python3 - "$out" <<'EOF'
import csv, glob, os, sys
acc = {}
for f in sorted(glob.glob(os.path.join(sys.argv[1], "p*", "**", "*counter_collection.csv"), recursive=True)):
    with open(f) as fh:
        for row in csv.DictReader(fh):
            if "k_pairhmm" in row.get("Kernel_Name", ""):
                d = acc.setdefault(row["Counter_Name"], {})
                d[row["Dispatch_Id"]] = d.get(row["Dispatch_Id"], 0.0) + float(row["Counter_Value"])
for k in sorted(acc):
    print("%-40s %16.1f  (%d launches)" % (k, sum(acc[k].values()) / len(acc[k]), len(acc[k])))
EOF
