#!/usr/bin/env python3
"""Whole-path time of the wide-network route (step-2 pencils of 17 <= P = M + K - 1 <= 32: csrc/k_cov_wide.h, csrc/k_solve_wide.h,
k_apply_m<M, 31>), since bench.py's workloads stop at P = 15.  10 s signals (160 000 samples), oracle masks, synthetic rooms formed
on the device (disco_amd.synth.make_rooms_torch):
  W1  64 rooms x 16 nodes x 4 mics, P2 = 19        W2  16 rooms x 25 nodes x 8 mics, P2 = 32
Reports ms per step (median of --steps after --warmup, host clock around disco_tango_enhance + a device sync), x real-time, the stage split of
one more eager step (stage_timing), a byte / flop model of the new kernels, and the worst relative error of --check sampled rooms
against the float64 oracle (oracle/tango_oracle.py), asserted < 1e-4.

Model (per step; G = R K units, T frames, F bins, P = P2, NP = P (P + 1) / 2):
  cov2   bytes = G T F (8 M + 4) + R K T F 8 (every z row once per room through L2) + G chunks F NP 16 (the partial sums);
         flops = G T F NP 8 (two statistics, one complex multiply-add each: 4 real FMAs = 8 flops)
  solve2 float64 flops ~ 8 (P^3 / 6 + P^3 + s P^3) per pencil, s = 5 squarings (typical), G F pencils
  apply2 bytes = G T F (8 M + 8 + 8) + R K T F 8
Usage: wide_time.py [--workloads W1,W2] [--steps N] [--warmup N] [--check N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from disco_amd import synth  # noqa: E402
from disco_amd.engine import Engine  # noqa: E402

WORKLOADS = {'W1': dict(rooms=64, nodes=16, mics=4), 'W2': dict(rooms=16, nodes=25, mics=8)}
L, FS = 160000, 16000
HBM_GBPS, F64_TFLOPS = 8000.0, 78.6          # MI355X peak HBM bandwidth and float64 vector rate


def run(name, steps, warmup, check):
    w = WORKLOADS[name]
    R, K, M = w['rooms'], w['nodes'], w['mics']
    P = M + K - 1
    eng = Engine(rooms=R, nodes=K, mics=M, length=L)
    y, s, n = synth.make_rooms_torch(R, K=K, M=M, L=L, ref_only_sn=not check)
    s0, n0 = (s[:, :, 0], n[:, :, 0]) if check else (s, n)
    mask = eng.mask_oracle(s0.reshape(R * K, L).contiguous(), n0.reshape(R * K, L).contiguous()).reshape(R, K, eng.T, eng.F)
    T, F = eng.T, eng.F
    out = torch.empty((R, K, L), dtype=torch.float32, device='cuda')

    def step():
        return eng.tango_enhance(y, mask, want_z=False, want_yf=False, out=out)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    eng.sync()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        eng.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(ts))
    eng.stage_timing(True)
    step()
    stages = eng.stage_report()
    eng.stage_timing(False)
    G, NP = R * K, P * (P + 1) // 2
    chunks = max(1, min(8, (2048 + G - 1) // G, T))
    cov_b = G * T * F * (8 * M + 4) + G * T * F * 8 + G * chunks * F * NP * 16
    cov_f = G * T * F * NP * 8
    solve_f = G * F * 8 * (P ** 3 / 6 + P ** 3 + 5 * P ** 3)
    apply_b = G * T * F * (8 * M + 16) + G * T * F * 8
    row = {'workload': name, 'rooms': R, 'nodes': K, 'mics': M, 'P2': P, 'T': T, 'F': F, 'ms_per_step': ms, 'ms_min': float(np.min(ts)),
           'steps': steps,
           'stages_ms': {k: v[0] for k, v in stages.items()}, 'model': {}}
    row['x_realtime'] = (L / FS) / (ms / 1e3)            # seconds of audio of every node per second of wall time
    st = row['stages_ms']
    if 'cov2' in st:
        row['model']['cov2'] = {'bytes': cov_b, 'flops': cov_f, 'hbm_frac': cov_b / (st['cov2'] * 1e-3) / (HBM_GBPS * 1e9),
                                'fp32_tflops': cov_f / (st['cov2'] * 1e-3) / 1e12}
    if 'solve2' in st:
        row['model']['solve2'] = {'flops_f64': solve_f, 'f64_frac': solve_f / (st['solve2'] * 1e-3) / (F64_TFLOPS * 1e12),
                                  'pencils': G * F}
    if 'apply2' in st:
        row['model']['apply2'] = {'bytes': apply_b, 'hbm_frac': apply_b / (st['apply2'] * 1e-3) / (HBM_GBPS * 1e9)}
    # sampled rooms against the float64 oracle
    if check:
        from oracle import stft_oracle as so
        from oracle import tango_oracle as to
        got = out.cpu().numpy()
        worst = 0.0
        for r in np.linspace(0, R - 1, check).astype(int):
            yr, sr, nr = (t[r].cpu().numpy() for t in (y, s, n))         # the very inputs the timed steps ran on
            o = to.offline_tango_vec(yr, sr, nr, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
            for k in range(K):
                ref = so.istft(o['yf'][k], L, 512, 256, work_dtype=np.float64)
                worst = max(worst, float(np.linalg.norm(got[r, k] - ref) / np.linalg.norm(ref)))
        row['parity'] = {'rooms_checked': int(check), 'worst_rel': worst, 'tol': 1e-4, 'ok': worst < 1e-4}
        assert worst < 1e-4, row
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', default='W1,W2')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--check', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = [run(w, args.steps, args.warmup, args.check) for w in args.workloads.split(',')]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
