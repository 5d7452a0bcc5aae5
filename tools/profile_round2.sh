#!/bin/bash
# Round-2 measurement set on the GPU box (run through gpurun): GPU tests, bench line, rocprofv3 kernel stats of the same command,
# the two HBM-traffic PMC passes, one SQ (MFMA utilisation) pass, kernel stats of the secondary configs, a step timeline.
# Outputs under gpurun_out/; the summaries are copied to profiles/ (tracked).   usage: bash tools/profile_round2.sh <tag> [notest]
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out; T=${1:-r02}
cd $R
if [ "$2" != "notest" ]; then timeout 1500 python -m pytest tests -q -m gpu -x > $O/pytest_$T.log 2>&1; tail -3 $O/pytest_$T.log; fi
python bench.py --steps 20 --warmup 5 --full > $O/bench_$T.json 2> $O/bench_$T.err; tail -c 600 $O/bench_$T.json; echo
cd /tmp && export TMPDIR=/tmp
rm -rf $O/prof_$T; rocprofv3 --kernel-trace --stats -d $O/prof_$T -o $T --output-format csv -- python3 $R/bench.py --steps 20 --warmup 5 --no-cpu-baseline --aux "" > $O/prof_${T}_bench.log 2>&1
find $O/prof_$T -name "*kernel_trace.csv" -delete
for c in FETCH_SIZE WRITE_SIZE; do rm -rf $O/pmc_$c; rocprofv3 --pmc $c --kernel-trace -d $O/pmc_$c -o p --output-format csv -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --aux "" > $O/pmc_$c.log 2>&1; f=$(find $O/pmc_$c -name "*counter_collection.csv" | head -1); python3 $R/tools/pmc_summary.py $f $c > $O/pmc_$c.json; rm -rf $O/pmc_$c; done
python3 $R/tools/pmc_merge.py $O/pmc_FETCH_SIZE.json $O/pmc_WRITE_SIZE.json $O/${T}_pmc_traffic.json > /dev/null
rm -rf $O/pmc_sq; rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_VALU_MFMA_MOPS_F32 GRBM_GUI_ACTIVE --kernel-trace -d $O/pmc_sq -o p --output-format csv -- python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --aux "" > $O/pmc_sq.log 2>&1
f=$(find $O/pmc_sq -name "*counter_collection.csv" | head -1); python3 $R/tools/pmc_mfma.py $f $O/${T}_pmc_mfma.json; rm -rf $O/pmc_sq
for c in c1 c2 c2bf16 c5; do
  rm -rf $O/prof_$c; rocprofv3 --kernel-trace --stats -d $O/prof_$c -o ${T}_$c --output-format csv -- python3 $R/bench.py --aux-child $c > $O/prof_$c.log 2>&1
  find $O/prof_$c -name "*kernel_trace.csv" -delete
done
rm -rf $O/prof_tl; rocprofv3 --kernel-trace -d $O/prof_tl -o tl --output-format rocpd -- python3 $R/bench.py --steps 8 --warmup 3 --no-cpu-baseline --aux "" > $O/prof_tl.log 2>&1
db=$(find $O/prof_tl -name "*.db" | head -1); [ -n "$db" ] && python3 $R/tools/timeline.py $db 60e3 > $O/${T}_timeline.txt 2>&1; rm -rf $O/prof_tl
ls $O | head -50
