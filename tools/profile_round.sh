#!/bin/bash
# Run on the GPU box (through gpurun): rocprofv3 kernel stats + the two PMC passes behind bench.py's roofline object.
# Usage: tools/profile_round.sh <tag> [bench args, e.g. --config C5]
#   -> $OUT/<tag>_kernel_stats.csv, $OUT/<tag>_pmc_raw.json, $OUT/<tag>_pmc_traffic.json
TAG=${1:-r02}
shift
ARGS="$@"
cd /tmp; export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the directory the outputs go to}; mkdir -p $OUT
DISCO_OVERLAP_SOLVES=0 timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o $TAG -- python bench.py $ARGS --extras none --steps 5 --warmup 2 --no-cpu-baseline --no-parity > $OUT/${TAG}_bench_under_rocprof.log 2>&1; echo "stats rc $?"
# (DISCO_OVERLAP_SOLVES=0: kernels one at a time, the mode bench.py takes its per-kernel roofline figure in)
# counters in their own runs, --kernel-trace only (the PMC + trace-domain combination is refused on this pool)
DISCO_OVERLAP_SOLVES=0 timeout 900 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_$TAG -o fetch -- python bench.py $ARGS --extras none --steps 1 --warmup 0 --no-cpu-baseline --no-stage-timing --no-parity --pmc-calibrate > $OUT/${TAG}_pmc_fetch.log 2>&1; echo "fetch rc $?"
DISCO_OVERLAP_SOLVES=0 timeout 900 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_$TAG -o write -- python bench.py $ARGS --extras none --steps 1 --warmup 0 --no-cpu-baseline --no-stage-timing --no-parity --pmc-calibrate > $OUT/${TAG}_pmc_write.log 2>&1; echo "write rc $?"
python tools/pmc_extract.py $OUT/${TAG}_pmc_raw.json FETCH_SIZE=$OUT/pmc_$TAG/fetch_results.db WRITE_SIZE=$OUT/pmc_$TAG/write_results.db
python tools/rocprof_summary.py $OUT/prof_$TAG/${TAG}_results.db $OUT/${TAG}_kernel_stats.csv
python tools/pmc_traffic.py $OUT/${TAG}_pmc_raw.json $OUT/${TAG}_pmc_traffic.json
rm -rf $OUT/pmc_$TAG $OUT/prof_$TAG
grep disco $OUT/${TAG}_kernel_stats.csv | cut -c1-120 | head -12
