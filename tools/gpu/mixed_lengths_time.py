#!/usr/bin/env python3
"""What a batch of rooms of DIFFERENT clip lengths costs (disco_set_lengths): the C3 shape (1000 rooms x 4 nodes x 4 mics, 512-point STFT,
arrays of 160 000 samples), oracle masks computed in the step, synthetic rooms formed on the device (disco_amd.synth.make_rooms_torch),
seeded lengths uniform on [80 000, 160 000].  In ONE process, alternated round by round so that both see the same box in the same state:
  (a) the uniform batch at 160 000 samples (no lengths set)
  (b) the mixed batch (the same arrays, lengths set)
Reports ms per step of both (median over all rounds, and the median of every round: their spread is the margin a difference has to
exceed), (c) = sum T_r / (R Tmax), the share of the rectangle's frames that exist, the per-stage split of one more eager step of each
(stage_timing), and the worst relative error of --check sampled rooms of the mixed batch against the float64 oracle run on each room
alone at its own length (oracle/tango_oracle.py), asserted < 1e-4.  The sampled rooms are taken among those whose length has
L % hop <= hop / 2 (nearer to a whole hop the last samples of ANY clip, uniform batch included, are divided by an almost-zero window sum).
Usage: mixed_lengths_time.py [--rooms N] [--steps N] [--rounds N] [--warmup N] [--check N] [--out FILE]"""
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

K, M, L, N_FFT, HOP = 4, 4, 160000, 512, 256
L_LO = 80000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=10, help='timed steps per round and variant')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--check', type=int, default=3)
    ap.add_argument('--seed', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    R = args.rooms
    lengths = np.random.default_rng(args.seed).integers(L_LO, L + 1, R).astype(np.int32)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, n_fft=N_FFT)
    eng.reserve(1)
    T, F = eng.T, eng.F
    y, s, n = synth.make_rooms_torch(R, K=K, M=M, L=L, ref_only_sn=not args.check)
    s0, n0 = (s[:, :, 0].contiguous(), n[:, :, 0].contiguous()) if args.check else (s, n)
    mask = torch.empty((R, K, T, F), dtype=torch.float32, device='cuda')
    out = torch.empty((R, K, L), dtype=torch.float32, device='cuda')
    lib = eng.lib

    def step():
        eng._chk(lib.disco_mask_oracle(eng.ctx, s0.data_ptr(), n0.data_ptr(), R * K, mask.data_ptr(), eng.stream))
        eng.tango_enhance(y, mask, want_z=False, want_yf=False, out=out)

    def timed(steps):
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            eng.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    variants = {'uniform': None, 'mixed': lengths}
    times = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for name, lens in variants.items():
            eng.set_lengths(lens)
            for _ in range(args.warmup if rnd == 0 else 1):
                step()
            eng.sync()
            times[name].append(timed(args.steps))
    stages = {}
    for name, lens in variants.items():
        eng.set_lengths(lens)
        step()
        eng.sync()
        eng.stage_timing(True)
        step()
        stages[name] = {k: v[0] for k, v in eng.stage_report().items()}
        eng.stage_timing(False)
    frames = 1 + lengths // HOP
    share = float(frames.sum() / (R * T))
    row = {'shape': {'rooms': R, 'nodes': K, 'mics': M, 'length': L, 'n_fft': N_FFT, 'T': T},
           'lengths': {'seed': args.seed, 'low': L_LO, 'high': L, 'mean': float(lengths.mean()), 'frame_share': share},
           'steps_per_round': args.steps, 'rounds': args.rounds}
    for name in variants:
        allt = np.concatenate(times[name])
        row[name] = {'ms_per_step': float(np.median(allt)), 'ms_min': float(allt.min()),
                     'round_medians_ms': [float(np.median(t)) for t in times[name]], 'stages_ms': stages[name]}
    a, b = row['uniform']['ms_per_step'], row['mixed']['ms_per_step']
    row['mixed_over_uniform'] = b / a
    row['towards_frame_share'] = (a - b) / (a - share * a) if share < 1 else None       # 1: the mixed batch pays for its frames only
    if args.check:
        from oracle import stft_oracle as so
        from oracle import tango_oracle as to
        eng.set_lengths(lengths)
        step()
        eng.sync()
        got = out.cpu().numpy()
        ok_rooms = [r for r in range(R) if lengths[r] % HOP <= HOP // 2]
        picks = [ok_rooms[i] for i in np.linspace(0, len(ok_rooms) - 1, args.check).astype(int)]
        worst, zeros = 0.0, True
        for r in picks:
            Lr = int(lengths[r])
            yr, sr, nr = (t[r, :, :, :Lr].cpu().numpy() for t in (y, s, n))        # the very inputs the timed steps ran on
            o = to.offline_tango_vec(yr, sr, nr, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
            zeros = zeros and not got[r, :, Lr:].any()
            for k in range(K):
                ref = so.istft(o['yf'][k], Lr, N_FFT, HOP, work_dtype=np.float64)
                worst = max(worst, float(np.linalg.norm(got[r, k, :Lr] - ref) / np.linalg.norm(ref)))
        row['parity'] = {'rooms_checked': [int(r) for r in picks], 'lengths': [int(lengths[r]) for r in picks], 'worst_rel': worst,
                         'tol': 1e-4, 'padding_zero': bool(zeros), 'ok': bool(worst < 1e-4 and zeros)}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(row, open(args.out, 'w'), indent=1)
    if args.check:
        assert row['parity']['ok'], row['parity']


if __name__ == '__main__':
    main()
