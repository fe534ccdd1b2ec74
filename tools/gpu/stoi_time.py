#!/usr/bin/env python3
"""Time of the STOI scoring (disco_stoi, csrc/k_stoi.h) at the reference's rate and span (16 kHz, L = 144 000 samples scored: 10 s minus
the first second).

What room_results(stoi=True) does per room of 4 nodes is timed as it is issued: 24 pairs per room (3 processed signals x 2 clean
signals x 4 nodes).  --rooms rooms are scored in one Engine.stoi call on device-resident float32 signals (speech-like clean signals of
tests/stoi_checks.py, processed = clean + white noise at 5 dB: silent-frame removal does happen) and the figures for 1000 rooms are the
per-room figures times 1000 -- stated as an extrapolation.  Kernel times are hipEvent pairs around the launches of each of the four
stages (disco_stage_timing: stoi_resample, stoi_frames, stoi_tob, stoi_corr), summed per stage; a warm-up call, then --reps calls,
median and min / max over the calls.  For scale: the wall time of the float64 yardstick (tests/stoi_checks.py, its whole-array form and
its loops) on one pair.
Usage: stoi_time.py [--rooms N] [--reps N] [--out FILE]"""
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
STAGES = ('stoi_resample', 'stoi_frames', 'stoi_tob', 'stoi_corr')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=25)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import stoi_checks as sc
    eng = Engine(rooms=1, nodes=1, mics=1, length=1024)
    R = args.rooms
    n_pair = R * PAIRS_PER_ROOM
    base = [sc.make_pair(seed, L, FS_SIG, 5.0) for seed in sc.SEEDS]
    g = torch.Generator(device='cuda').manual_seed(0)
    x = torch.stack([torch.from_numpy(base[i % 3][0]) for i in range(n_pair)]).cuda()
    y = (x + 0.05 * torch.randn((n_pair, L), generator=g, device='cuda')).contiguous()
    eng.stoi(x, y, FS_SIG)                                                    # warm-up
    wall, stages = [], []
    for _ in range(args.reps):
        eng.stage_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d, st = eng.stoi(x, y, FS_SIG)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append({k: v[0] for k, v in eng.stage_report().items()})
        eng.stage_timing(False)
    assert not st.any() and np.all(np.isfinite(d))
    row = {'rooms': R, 'pairs': n_pair, 'fs_sig': FS_SIG, 'L': L, 'reps': args.reps, 'wall_ms_median': float(np.median(wall)),
           'wall_ms_min': float(np.min(wall)), 'wall_ms_max': float(np.max(wall)), 'd_min': float(d.min()), 'd_max': float(d.max())}
    for name in STAGES:
        ts = [s_[name] for s_ in stages]
        row[name] = {'ms_median': float(np.median(ts)), 'ms_min': float(np.min(ts)), 'ms_max': float(np.max(ts))}
    print(json.dumps(row), flush=True)
    per_room = row['wall_ms_median'] / R
    kern_room = sum(row[n]['ms_median'] for n in STAGES) / R
    summary = {'per_room_wall_ms': per_room, 'per_room_kernel_ms': kern_room, 'extrapolated_1000_rooms_wall_s': per_room,
               'extrapolated_1000_rooms_kernel_s': kern_room}
    xh, yh = base[0]
    t0 = time.perf_counter()
    sc.stoi_vectorised(xh, yh, FS_SIG)
    summary['cpu_yardstick_vectorised_one_pair_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sc.stoi_yardstick(xh, yh, FS_SIG)
    summary['cpu_yardstick_loops_one_pair_s'] = time.perf_counter() - t0
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({'runs': [row], 'summary': summary}, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
