#!/usr/bin/env python3
"""What a CRNN-mask batch of rooms of DIFFERENT clip lengths costs (dnn/inloop.py:tango_enhance_dnn with Engine.set_lengths): the C4 shape
(125 rooms x 4 nodes x 4 mics, 512-point STFT, arrays of 160 000 samples = 10 s), two seeded networks (output layer spread as bench.py
does), synthetic rooms formed on the device, seeded lengths uniform on [80 000, 160 000] (5 s ... 10 s).  In ONE process, alternated round by
round so that both see the same box in the same state:
  (a) the uniform batch at 160 000 samples (no lengths set)
  (b) the mixed batch (the same arrays, lengths set)
Events on the launch stream after every phase (tango_enhance_dnn's `mark`): per-phase tables of both (median over all timed steps), the step
as the sum of its phases, and N / (B T) = sum T_r / (R Tmax), the share of the rectangle's frames that exist -- the recurrent and output
layers (`crnn.flops_per_frame`: about 62 % of the one-channel network's multiply-adds) run on that share, the convolutions on all of it.
No bar: the uniform run of the same process is the yardstick.
Usage: crnn_lengths_time.py [--rooms N] [--steps N] [--rounds N] [--warmup N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from disco_amd import synth  # noqa: E402
from disco_amd.dnn.crnn import build_crnn  # noqa: E402
from disco_amd.dnn.inloop import tango_enhance_dnn  # noqa: E402
from disco_amd.engine import Engine  # noqa: E402

K, M, L, N_FFT, HOP = 4, 4, 160000, 512, 256
L_LO = 80000


class Marks:
    """an event on the launch stream after every phase"""

    def __init__(self):
        self.ev = []
        self('start')

    def __call__(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((name, e))

    def phases(self):
        torch.cuda.synchronize()
        return {name: a.elapsed_time(b) for (_, a), (name, b) in zip(self.ev[:-1], self.ev[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=125)
    ap.add_argument('--steps', type=int, default=5, help='timed steps per round and variant')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'crnn_lengths_time.json'))
    args = ap.parse_args()
    R = args.rooms
    dev = torch.device('cuda', 0)
    lengths = np.random.default_rng(args.seed).integers(L_LO, L + 1, R).astype(np.int32)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, n_fft=N_FFT)
    T = eng.T
    y = synth.make_rooms_torch(R, K=K, M=M, L=L, device=dev, ref_only_sn=True)[0]
    torch.manual_seed(0)
    model_z, model_w = build_crnn(1, device=dev), build_crnn(K, device=dev)
    with torch.no_grad():
        for mdl in (model_z, model_w):
            mdl.ff.layers[0].weight.mul_(40.0)

    def step(mark=None):
        return tango_enhance_dnn(eng, y, model_z, model_w, mark=mark)

    variants = {'uniform': None, 'mixed': lengths}
    tables = {k: [] for k in variants}
    for rnd in range(args.rounds):
        for name, lens in variants.items():
            eng.set_lengths(lens)
            for _ in range(args.warmup if rnd == 0 else 1):
                step()
            torch.cuda.synchronize()
            for _ in range(args.steps):
                marks = Marks()
                step(marks)
                tables[name].append(marks.phases())
    eng.set_lengths(None)
    frames = 1 + lengths // HOP
    share = float(frames.sum() / (R * T))
    row = {'shape': {'rooms': R, 'nodes': K, 'mics': M, 'length': L, 'n_fft': N_FFT, 'T': T, 'signals': R * K},
           'lengths': {'seed': args.seed, 'low': L_LO, 'high': L, 'mean': float(lengths.mean()), 'frame_share': share},
           'steps_per_round': args.steps, 'rounds': args.rounds}
    for name in variants:
        names = list(tables[name][0])
        med = {p: float(np.median([t[p] for t in tables[name]])) for p in names}
        totals = [sum(t.values()) for t in tables[name]]
        row[name] = {'phases_ms': med, 'ms_per_step': float(np.median(totals)), 'ms_min': float(min(totals)),
                     'round_medians_ms': [float(np.median(totals[i * args.steps:(i + 1) * args.steps])) for i in range(args.rounds)]}
    row['mixed_over_uniform'] = {p: row['mixed']['phases_ms'][p] / row['uniform']['phases_ms'][p] for p in row['uniform']['phases_ms']}
    row['mixed_over_uniform']['step'] = row['mixed']['ms_per_step'] / row['uniform']['ms_per_step']
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(row, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
