#!/bin/bash
# FINAL-state pass of a round on the committed sources (round 4: r4_final.sh): GPU suite, the `bench.py --full` line, kernel stats + HBM counters (+ calibration) of
# C3 / C5 / C2 / C2x4000, SQ / LDS counters of C3 / C5, side lines (overlap off, node-sharded, online every 8).   Usage: final_pass.sh <tag>
# PART=a: the suite and the --full line only; PART=b: the profile / counter passes and the side lines only (two calls when the GPU budget is short);
# PART=c: whole batches of C3 / C5 / C4 against the float64 oracle (bench.py --parity-rooms = the batch).  OUT: the directory the outputs go to
TAG=${1:-r06_zz}
PART=${PART:-ab}
cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
OUT=${OUT:?set OUT to the directory the outputs go to}; export OUT; mkdir -p $OUT
T0=$(date +%s)
if [[ $PART == *a* ]]; then
timeout 1500 python -m pytest tests -m gpu -q > $OUT/${TAG}_tests.log 2>&1; echo "tests rc $? ($(( $(date +%s) - T0 )) s)"; grep -E "passed|failed" $OUT/${TAG}_tests.log | tail -2; grep -E "^FAILED|^E  " $OUT/${TAG}_tests.log | head -10
T1=$(date +%s)
timeout 900 python bench.py --full --detail $OUT/${TAG}_bench_detail.json > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err; echo "bench rc $? ($(( $(date +%s) - T1 )) s)"; tail -3 $OUT/${TAG}_bench_default.err
python - <<PY
import json
line = open('$OUT/${TAG}_bench_default.json').read().strip().splitlines()[-1]
print('stdout line:', len(line), 'bytes; keys', list(json.loads(line)))
d = json.load(open('$OUT/${TAG}_bench_detail.json'))
print('C3', round(d['ms_per_step'], 3), 'ms', d['roofline']['kernel'], d['roofline']['frac'], 'pipe', d['roofline']['pipeline']['frac'], 'parity', d['parity_sample'] and d['parity_sample']['worst_rel_all_ranks'], d['roofline'].get('sanity_errors'))
print('   ', {s: x['ms'] for s, x in d['stages'].items()})
for k, v in d.get('configs', {}).items():
    if 'error' in v:
        print(k, 'ERROR', v['error'][:300]); continue
    rf = v.get('roofline') or {}
    print(k, round(v['ms_per_step'], 3), 'ms', 'xRT', round(v['x_realtime'], 1), rf.get('kernel', '')[:40], rf.get('frac'), 'pipe', (rf.get('pipeline') or {}).get('frac'), 'parity', (v.get('parity_sample') or {}).get('worst_rel_all_ranks'), 'ok', (v.get('parity_sample') or {}).get('ok'), rf.get('sanity_errors'))
    print('   ', {s: x['ms'] for s, x in (v.get('stages') or {}).items()})
PY
fi
if [[ $PART == *b* ]]; then
bash tools/profile_round.sh ${TAG}_C3 2>&1 | tail -9
bash tools/profile_round.sh ${TAG}_C5 --config C5 2>&1 | tail -12
bash tools/profile_round.sh ${TAG}_C2 --config C2 2>&1 | tail -6
bash tools/profile_round.sh ${TAG}_C2x4000 --config C2 --rooms 4000 2>&1 | tail -6
if [[ -z "$SKIP_ALU" ]]; then
BARGS="" bash tools/gpu/pmc_alu.sh ${TAG}_C3 2>&1 | grep -E "rc|disco::" | cut -c1-400
BARGS="--config C5" bash tools/gpu/pmc_alu.sh ${TAG}_C5 2>&1 | grep -E "rc|disco::" | cut -c1-400
fi
BARGS="--rooms 1000 --online-every 1" bash tools/gpu/pmc_alu.sh ${TAG}_online1 2>&1 | grep -E "rc|disco::" | cut -c1-400
python - <<PY
# the online mode's VALU-issue roofline reads this copy (bench.py: profiles/pmc_alu_online1.json), stamped with the digest of the kernel sources
import json, sys
sys.path.insert(0, '.')
import bench
d = json.load(open('$OUT/${TAG}_online1_pmc_alu.json'))
d['_csrc_digest'] = bench.csrc_digest()
json.dump(d, open('$OUT/pmc_alu_online1.json', 'w'), indent=1)
PY
DISCO_OVERLAP_SOLVES=0 timeout 300 python bench.py --full --extras none --no-cpu-baseline > $OUT/${TAG}_bench_C3_overlap0.json 2>/dev/null
timeout 300 python bench.py --full --shard nodes --rooms 250 --extras none --no-cpu-baseline > $OUT/${TAG}_bench_nodeshard.json 2>/dev/null
timeout 300 python bench.py --full --rooms 1000 --online-every 8 --steps 2 --warmup 1 --extras none --no-cpu-baseline > $OUT/${TAG}_bench_online8.json 2>/dev/null
python - <<PY
import json
for n in ('C3_overlap0', 'nodeshard', 'online8'):
    try:
        d = json.loads(open(f'$OUT/${TAG}_bench_{n}.json').read().strip().splitlines()[-1])
        print(n, round(d['ms_per_step'], 3), 'ms xRT', round(d['x_realtime'], 1), 'parity', (d.get('parity_sample') or {}).get('worst_rel_all_ranks'))
    except Exception as e:
        print(n, 'failed', e)
PY
fi
if [[ $PART == *c* ]]; then
# whole batches against the float64 oracle (many oracle workers: the box has them), one workload at a time
IFS=";" read -ra SW <<< "${SWEEPS:-C3 1000;C5 200;C4 125}"
for W in "${SW[@]}"; do
  set -- $W
  timeout 1500 python bench.py --full --config $1 --parity-rooms $2 --parity-workers 48 --steps 2 --warmup 1 --extras none --no-cpu-baseline --no-stage-timing --detail $OUT/${TAG}_sweep_$1.json > /dev/null 2> $OUT/${TAG}_sweep_$1.err; echo "sweep $1 rc $?"
  python tools/gpu/parity_hist.py $OUT/${TAG}_sweep_$1.json $OUT/${TAG}_parity_$1_all_$2.json | cut -c1-600
  rm -f $OUT/${TAG}_sweep_$1.json
done
fi
echo "total $(( $(date +%s) - T0 )) s"
