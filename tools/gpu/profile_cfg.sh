# usage: bash tools/gpu/profile_cfg.sh <tag> <bench args...>   -> $OUT/<tag>_kernel_stats.csv
TAG=$1; shift
cd /tmp; export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:?set OUT to the directory the outputs go to}; mkdir -p $OUT
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o $TAG -- python bench.py --no-cpu-baseline --no-stage-timing "$@" > $OUT/${TAG}_bench.log 2>&1; echo "rc $?"
python tools/rocprof_summary.py $OUT/prof/${TAG}_results.db $OUT/${TAG}_kernel_stats.csv
rm -f $OUT/prof/${TAG}_results.db
grep disco $OUT/${TAG}_kernel_stats.csv | cut -c1-130
grep '^{' $OUT/${TAG}_bench.log | tail -1 | cut -c1-300
