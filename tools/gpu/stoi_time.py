#!/usr/bin/env python3
"""Time of the STOI and ESTOI scoring (disco_stoi, csrc/k_stoi.h; disco_estoi, csrc/k_estoi.h) at the reference's rate and span (16 kHz,
L = 144 000 samples scored: 10 s minus the first second).

What room_results(stoi=True) does per room of 4 nodes is timed as it is issued: 24 pairs per room (3 processed signals x 2 clean
signals x 4 nodes).  For every entry of --rooms that many rooms are scored in one Engine.stoi call and one Engine.estoi call on the same
device-resident float32 signals (speech-like clean signals of tests/stoi_checks.py, processed = clean + white noise at 5 dB: silent-frame
removal does happen), the two measures alternated call by call; the figures for 1000 rooms are the per-room figures of the largest batch
times 1000 -- stated as an extrapolation.  Kernel times are hipEvent pairs around the launches of each of the four stages
(disco_stage_timing: stoi_resample, stoi_frames, stoi_tob, and stoi_corr or estoi_corr), summed per stage; a warm-up call of each, then
--reps calls, median and min / max over the calls.  For scale: the wall time of the float64 yardsticks (tests/stoi_checks.py,
tests/estoi_checks.py, their whole-array forms and their loops) on one pair.
Usage: stoi_time.py [--rooms N [N ...]] [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from disco_amd.engine import Engine  # noqa: E402

FS_SIG, L, K, PAIRS_PER_ROOM = 16000, 144000, 4, 24
SHARED = ('stoi_resample', 'stoi_frames', 'stoi_tob')
MEASURES = {'stoi': SHARED + ('stoi_corr',), 'estoi': SHARED + ('estoi_corr',)}


def time_batch(eng, base, R, reps):
    """-> {measure: row} for R rooms: the two measures alternated on one batch."""
    n_pair = R * PAIRS_PER_ROOM
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.stack([torch.from_numpy(base[i % 3][0]) for i in range(n_pair)]).cuda()
    y = (x + 0.05 * torch.randn((n_pair, L), generator=g, device='cuda')).contiguous()
    wall, stages, last = {m: [] for m in MEASURES}, {m: [] for m in MEASURES}, {}
    for m in MEASURES:
        getattr(eng, m)(x, y, FS_SIG)                                         # warm-up
    for _ in range(reps):
        for m in MEASURES:
            eng.stage_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[m] = getattr(eng, m)(x, y, FS_SIG)
            wall[m].append((time.perf_counter() - t0) * 1e3)
            stages[m].append({k: v[0] for k, v in eng.stage_report().items()})
            eng.stage_timing(False)
    rows = {}
    for m, names in MEASURES.items():
        d, st = last[m]
        assert not st.any() and np.all(np.isfinite(d))
        row = {'measure': m, 'rooms': R, 'pairs': n_pair, 'fs_sig': FS_SIG, 'L': L, 'reps': reps, 'wall_ms_median': float(np.median(wall[m])),
               'wall_ms_min': float(np.min(wall[m])), 'wall_ms_max': float(np.max(wall[m])), 'd_min': float(d.min()), 'd_max': float(d.max())}
        for name in names:
            ts = [s_[name] for s_ in stages[m]]
            row[name] = {'ms_median': float(np.median(ts)), 'ms_min': float(np.min(ts)), 'ms_max': float(np.max(ts))}
        row['kernel_ms_median'] = sum(row[n]['ms_median'] for n in names)
        print(json.dumps(row), flush=True)
        rows[m] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, nargs='+', default=[1, 25])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import estoi_checks as ec
    import stoi_checks as sc
    eng = Engine(rooms=1, nodes=1, mics=1, length=1024)
    base = [sc.make_pair(seed, L, FS_SIG, 5.0) for seed in sc.SEEDS]
    runs = [time_batch(eng, base, R, args.reps) for R in sorted(args.rooms)]
    summary = {}
    for m, row in runs[-1].items():
        R = row['rooms']
        summary[m] = {'per_room_wall_ms': row['wall_ms_median'] / R, 'per_room_kernel_ms': row['kernel_ms_median'] / R,
                      'extrapolated_1000_rooms_wall_s': row['wall_ms_median'] / R, 'extrapolated_1000_rooms_kernel_s': row['kernel_ms_median'] / R}
    xh, yh = base[0]
    for name, fn in (('stoi_vectorised', sc.stoi_vectorised), ('stoi_loops', sc.stoi_yardstick), ('estoi_vectorised', ec.estoi_vectorised),
                     ('estoi_loops', ec.estoi_yardstick)):
        t0 = time.perf_counter()
        fn(xh, yh, FS_SIG)
        summary[f'cpu_yardstick_{name}_one_pair_s'] = time.perf_counter() - t0
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({'runs': [row for r in runs for row in r.values()], 'summary': summary}, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
