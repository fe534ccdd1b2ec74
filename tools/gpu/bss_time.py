#!/usr/bin/env python3
"""Time of the BSS-eval scoring (disco_bss_eval, csrc/k_bss.h) at the reference's filter length (512 taps) and clip length
(L = 144 000 samples scored: 10 s minus the first second), with the achieved float64 rate per kernel.

What room_results does per room of 4 nodes is timed as it is issued: the `_cnv` keys are 4 reference sets of 2 sources with 3 estimate
sets each, the `_dry` keys 1 reference set with 12 estimate sets.  --rooms rooms are scored in one Engine.bss_eval call per kind on
device-resident float32 signals (white references, estimates = mixtures + noise: the kernels' work does not depend on the values) and
the figures for 1000 rooms are the per-room figures times 1000 -- stated as an extrapolation, the batch is walked in workspace chunks of
about 100 sets either way.  Kernel times are hipEvent pairs around the launches of every stage (disco_stage_timing), summed per stage;
a warm-up call, then --reps calls, median and min / max over the calls.  For scale: the wall time of the float64 CPU oracle
(tests/bss_checks.py: gram_oracle) on the six calls of one node.

FLOPs (real float64 operations, multiply-add = 2):
  correlation  2 flen L per signal pair; pairs per call = n_set nsrc^2 (references) + n_set n_est nsrc^2 (estimates)
  factor       N^3 / 3 per factorisation, N = nsrc flen for job 0 and flen for each of the nsrc - 1 diagonal blocks
  project      N^2 per right-hand side and job (forward substitution), nsrc right-hand sides per estimate set
No fraction of peak is claimed: no float64 peak of this part has been measured here.
Usage: bss_time.py [--rooms N] [--reps N] [--out FILE]"""
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

FLEN, L, NSRC, K = 512, 144000, 2, 4


def flops(n_set, n_est):
    corr = 2.0 * FLEN * L * (n_set * NSRC ** 2 * (1 + n_est))
    n0 = NSRC * FLEN
    factor = n_set * (n0 ** 3 / 3.0 + (NSRC - 1) * FLEN ** 3 / 3.0)
    project = n_set * n_est * NSRC * (n0 ** 2 + (NSRC - 1) * FLEN ** 2)
    return {'bss_corr': corr, 'bss_factor': factor, 'bss_project': project}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=25)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    eng = Engine(rooms=1, nodes=1, mics=1, length=1024)
    g = torch.Generator(device='cuda').manual_seed(0)
    R = args.rooms
    rows = []
    for kind, n_set, n_est in (('cnv', R * K, 3), ('dry', R, 3 * K)):
        refs = torch.randn((n_set, NSRC, L), generator=g, device='cuda')
        ests = (refs.sum(1, keepdim=True)[:, None] * 0.7 + 0.1 * torch.randn((n_set, n_est, NSRC, L), generator=g, device='cuda')).contiguous()
        eng.bss_eval(refs, ests, flen=FLEN)                                  # warm-up
        wall, stages = [], []
        for _ in range(args.reps):
            eng.stage_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            en, st = eng.bss_eval(refs, ests, flen=FLEN)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append({k: v[0] for k, v in eng.stage_report().items()})
            eng.stage_timing(False)
        assert not st.any() and np.all(np.isfinite(en))
        fl = flops(n_set, n_est)
        row = {'kind': kind, 'rooms': R, 'n_set': n_set, 'n_est': n_est, 'flen': FLEN, 'L': L, 'reps': args.reps,
               'wall_ms_median': float(np.median(wall)), 'wall_ms_min': float(np.min(wall)), 'wall_ms_max': float(np.max(wall))}
        for name in ('bss_corr', 'bss_factor', 'bss_project'):
            ts = [s_[name] for s_ in stages]
            ms = float(np.median(ts))
            row[name] = {'ms_median': ms, 'ms_min': float(np.min(ts)), 'ms_max': float(np.max(ts)), 'flops': fl[name],
                         'fp64_tflops': fl[name] / (ms * 1e-3) / 1e12}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del refs, ests
    per_room = sum(r['wall_ms_median'] for r in rows) / R
    kern_room = sum(r[n]['ms_median'] for r in rows for n in ('bss_corr', 'bss_factor', 'bss_project')) / R
    summary = {'per_room_wall_ms': per_room, 'per_room_kernel_ms': kern_room, 'extrapolated_1000_rooms_wall_s': per_room,
               'extrapolated_1000_rooms_kernel_s': kern_room}
    import bss_checks as bc
    r, e = bc.make_case('white', L, 2)
    t0 = time.perf_counter()
    bc.gram_oracle(r, e[0], 0, FLEN)
    one = time.perf_counter() - t0
    summary['cpu_gram_oracle_one_call_s'] = one
    summary['cpu_gram_oracle_one_node_s'] = 6 * one                           # six bss_eval_sources calls per node (tango.py:552-564)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({'runs': rows, 'summary': summary}, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
