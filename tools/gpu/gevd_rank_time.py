#!/usr/bin/env python3
"""Per-launch time of the rank-R GEVD-MWF solve (disco_gevd_mwf, csrc/k_gevd_full.h) at ranks 1, 2 and P, beside the rank-1 solver
(disco_gevd_mwf_r1) on the same inputs, with the achieved float64 rate.

Shapes: 1 028 000 pencils at P = 4 and P = 7 (C3's step-1 and step-2 solves), 820 800 at P = 15 (C5).  Device events around every
launch on the default stream (the engine's), a warm-up, the median of --reps launches.  Inputs are covariance-like pencils (a rank-1
target plus diffuse noise, 64 frames), formed on the device.

FLOPs per pencil (real float64 operations; a complex multiply-add is 8): Cholesky 8 P^3 / 6; whitening (two triangular solves of P
right-hand sides) 8 P^3; Jacobi 30 P^2 (P - 1) per sweep (P (P - 1) / 2 rotations, each updating 2 columns and 2 rows of C and 2
columns of V: 6 P complex entries at ~10 operations each); filters 24 P^2 (two back substitutions and the assembly).  The sweep count is
that of the same cyclic Jacobi with the same stopping rule run in numpy on a sample of the inputs (the kernel's own count is not
observable from outside); the rate is therefore an estimate of the useful work, not an instruction count.
Usage: gevd_rank_time.py [--reps N] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from disco_amd.engine import Engine  # noqa: E402

SHAPES = ((4, 1028000), (7, 1028000), (15, 820800))
TOL2 = 1e-26          # DISCO_JACOBI_TOL2
SWEEPS_MAX = 12       # DISCO_JACOBI_SWEEPS


def pencils(n, P, T=64, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)

    def cn(*s):
        return torch.complex(torch.randn(*s, generator=g, device='cuda'), torch.randn(*s, generator=g, device='cuda'))
    Rxx = torch.empty((n, P, P), dtype=torch.complex64, device='cuda')
    Rnn = torch.empty_like(Rxx)
    for a in range(0, n, 65536):            # in slices: the (n, P, T) intermediates of C5 would not fit at once
        b = min(n, a + 65536)
        m = b - a
        X = cn(m, P, 1) * cn(m, 1, T) + 0.3 * cn(m, P, T)
        N = cn(m, P, T)
        Rxx[a:b] = X @ X.conj().transpose(1, 2) / T
        Rnn[a:b] = N @ N.conj().transpose(1, 2) / T
    return Rxx.contiguous(), Rnn.contiguous()


def jacobi_sweeps(Rxx, Rnn):
    """Sweeps the kernel's stopping rule needs per pencil: cyclic complex Jacobi on C = L^-1 Rxx L^-H in numpy (float64)."""
    Rxx = np.asarray(Rxx, np.complex128)
    Rnn = np.asarray(Rnn, np.complex128)
    Li = np.linalg.inv(np.linalg.cholesky(Rnn))
    C = Li @ Rxx @ np.conjugate(np.swapaxes(Li, -1, -2))
    C = 0.5 * (C + np.conjugate(np.swapaxes(C, -1, -2)))
    n, P, _ = C.shape
    sweeps = np.zeros(n, int)
    done = np.zeros(n, bool)
    for s in range(SWEEPS_MAX):
        a2 = np.abs(C) ** 2
        fro = a2.sum((1, 2))
        off = (a2 * (1 - np.eye(P))).sum((1, 2))                   # summed directly, as the kernel does (no cancellation)
        done |= ~(off > TOL2 * fro)
        if done.all():
            break
        sweeps[~done] += 1
        for p in range(P):
            for q in range(p + 1, P):
                b = C[:, p, q]
                rot = (b.real ** 2 + b.imag ** 2) > 1e-300                 # as the kernel: no rotation below
                ab = np.where(rot, np.abs(b), 1.0)
                dd = C[:, q, q].real - C[:, p, p].real
                t = np.where(rot, 2 * ab / (np.abs(dd) + np.sqrt(dd * dd + 4 * ab * ab)), 0.0)
                e = np.where(rot, b / ab, 1.0)
                t = np.where(dd < 0, -t, t)
                c = 1 / np.sqrt(1 + t * t)
                s_ = t * c
                J = np.zeros((n, 2, 2), complex)
                J[:, 0, 0], J[:, 0, 1], J[:, 1, 0], J[:, 1, 1] = c, s_, -s_ * np.conj(e), c * np.conj(e)
                J[done] = np.eye(2)
                idx = [p, q]
                C[:, :, idx] = C[:, :, idx] @ J
                C[:, idx, :] = np.conjugate(np.swapaxes(J, 1, 2)) @ C[:, idx, :]
                live = ~done
                C[live, p, q] = C[live, q, p] = 0                  # as the kernel: the annihilated pair exactly 0, the diagonal real
                C[live, p, p] = C[live, p, p].real
                C[live, q, q] = C[live, q, q].real
    return sweeps


def flops_per_pencil(P, sweeps):
    return 8 * P ** 3 / 6 + 8 * P ** 3 + 30 * P * P * (P - 1) * sweeps + 24 * P ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    eng = Engine(rooms=1, nodes=1, mics=1, length=1024)
    lib, ctx = eng.lib, eng.ctx
    rows = []
    for P, n in SHAPES:
        Rxx, Rnn = pencils(n, P)
        w = torch.empty((n, P), dtype=torch.complex64, device='cuda')
        t1 = torch.empty_like(w)
        sample = np.random.default_rng(0).choice(n, 512, replace=False)
        sw = jacobi_sweeps(Rxx[sample].cpu().numpy(), Rnn[sample].cpu().numpy())
        runs = {'r1': lambda: lib.disco_gevd_mwf_r1(ctx, Rxx.data_ptr(), Rnn.data_ptr(), n, P, ctypes.c_float(1.0), w.data_ptr(),
                                                    t1.data_ptr(), None)}
        for rank in (1, 2, P):
            runs[f'rank{rank}'] = (lambda r=rank: lib.disco_gevd_mwf(ctx, Rxx.data_ptr(), Rnn.data_ptr(), n, P, r, ctypes.c_float(1.0),
                                                                     w.data_ptr(), t1.data_ptr(), None))
        for name, fn in runs.items():
            for _ in range(3):
                assert fn() == 0, lib.disco_last_error(ctx)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                assert fn() == 0
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            ms = float(np.median(ts))
            row = {'P': P, 'n': n, 'route': name, 'ms_median': ms, 'ms_min': float(np.min(ts)), 'reps': args.reps}
            if name != 'r1':
                f = flops_per_pencil(P, float(sw.mean()))
                row.update(sweeps_mean=float(sw.mean()), sweeps_max=int(sw.max()), flops_per_pencil=f,
                           fp64_tflops=f * n / (ms * 1e-3) / 1e12)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
