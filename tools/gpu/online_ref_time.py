#!/usr/bin/env python3
"""What scoring the online mode costs: Engine.tango_online_reference (the mixture and both images through the per-frame filters, nine
spectra; with `signals` the six time signals too) against Engine.tango_online (the mixture alone) on the C3 shape -- 1000 rooms x 4
nodes x 4 microphones, 10-s clips -- with a filter update every frame and every 8 frames.

The rooms are white noise (the online kernels' time does not depend on the data: every frame is one solve).  Every figure is the median of
--reps calls timed with a pair of events on the stream after --warmup calls; min and max beside it.  The per-stage times of the
reference call come from disco_stage_report.
--parent-lib PATH: a libdisco_hip.so built from the parent commit; its tango_online is timed in the same process on the same inputs.
The two plain figures must agree within the box-to-box spread (+-3 %): the plain kernels are not to have moved.
Usage: online_ref_time.py [--rooms N] [--reps N] [--warmup N] [--parent-lib PATH] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from disco_amd import _lib  # noqa: E402
from disco_amd.engine import Engine  # noqa: E402

K, M, L = 4, 4, 160000


def bind_what_exists(path):
    """A library of another commit: the prototypes of the symbols it has."""
    cdll = ctypes.CDLL(path)
    for name, (res, args) in _lib.PROTOTYPES.items():
        if hasattr(cdll, name):
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = res, args
    return cdll


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    R = args.rooms
    g = torch.Generator(device='cuda').manual_seed(0)
    s = 0.2 * torch.randn((R, K, M, L), generator=g, device='cuda')
    n = 0.1 * torch.randn((R, K, M, L), generator=g, device='cuda')
    y = s + n
    eng = Engine(rooms=R, nodes=K, mics=M, length=L)
    eng.reserve(2)
    T, F = eng.T, eng.F
    mask = eng.mask_oracle(s[:, :, 0].reshape(R * K, L).contiguous(), n[:, :, 0].reshape(R * K, L).contiguous()).reshape(R, K, T, F)
    out = torch.empty((R, K, L), device='cuda')
    names = ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w')
    spec = {nm: torch.empty((R, K, T, F), dtype=torch.float32 if nm.startswith('mask') else torch.complex64, device='cuda') for nm in names}
    sig = torch.empty((6, R, K, L), device='cuda')
    outs = _lib.DiscoRefOutputs(**{nm: t.data_ptr() for nm, t in spec.items()})
    parent = None
    if args.parent_lib:
        parent = Engine(rooms=R, nodes=K, mics=M, length=L, lib=bind_what_exists(args.parent_lib))
        parent.reserve(1)
    report = {'rooms': R, 'nodes': K, 'mics': M, 'L': L, 'frames': T, 'reps': args.reps, 'warmup': args.warmup}
    for U in (1, 8):
        def plain(e):
            return lambda: e.tango_online(y, mask, update_every=U, want_z=False, want_yf=False, out=out)

        def ref(signals):
            def call():
                eng._chk(eng.lib.disco_tango_online_reference(eng.ctx, y.data_ptr(), s.data_ptr(), n.data_ptr(), None, None, 0.95, U, 1e-3,
                                                              ctypes.byref(outs), sig.data_ptr() if signals else None, None, 0, eng.stream))
            return call
        row = {}
        if parent is not None:
            row['tango_online_parent'] = timed(plain(parent), args.reps, args.warmup)
        row['tango_online'] = timed(plain(eng), args.reps, args.warmup)
        row['tango_online_reference'] = timed(ref(False), args.reps, args.warmup)
        row['tango_online_reference_signals'] = timed(ref(True), args.reps, args.warmup)
        base = row['tango_online']['ms_median']
        row['reference_over_plain'] = row['tango_online_reference']['ms_median'] / base
        row['reference_signals_over_plain'] = row['tango_online_reference_signals']['ms_median'] / base
        if parent is not None:
            row['plain_over_parent'] = base / row['tango_online_parent']['ms_median']
        for label, fn in (('stages_plain', plain(eng)), ('stages_reference_signals', ref(True))):
            eng.stage_timing(True)
            fn()
            eng.sync()
            row[label] = {k: round(v[0], 3) for k, v in eng.stage_report().items()}          # ms of one call, by stage
            eng.stage_timing(False)
        report[f'update_every_{U}'] = row
        print(json.dumps({f'update_every_{U}': row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(report, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
