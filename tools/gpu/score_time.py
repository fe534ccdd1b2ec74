#!/usr/bin/env python3
"""Time of scoring a batch of enhanced rooms: results_io.batch_results (one call for the batch, a stop per room) against the loop of
results_io.room_results over the same rooms (one call per room on host slices: the only way before batch_results existed).

C3-shaped rooms: K = 4 nodes, 10-s clips at 16 kHz (L = 160 000), clip lengths drawn uniformly in [5 s, 10 s], the first second skipped as
the reference does.  All eleven signals of the batch are device-resident float32 tensors (white targets and noises through short FIR
"rooms", enhanced versions = scaled images + a little noise, as tests/bss_checks.room_signals builds them): batch_results reads them in
place; the loop has to bring each room's signals to the host first (room_results slices on the host and copies the slices back), and
that copy is part of what it costs -- it is also reported on its own.

Three configurations, each timed for both routes after one warm-up call, --reps calls, median and min / max of the wall time (the calls
end on the host with the figures, so they are synchronous):
    levels        the fw_snr / fw_sd keys only (no y_in / sh_t / szh_t)
    bss           + the eleven BSS-eval keys at --flen taps (512: mir_eval's, what dominates)
    bss_stoi      + the STOI keys
--rooms is as many rooms as the run is given time for; the figures are for that many rooms and nothing is extrapolated.
Usage: score_time.py [--rooms N] [--reps N] [--flen N] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from disco_amd.speech_enhancement import results_io as rio  # noqa: E402

FS, L, K = 16000, 160000, 4
ROOM_KEYS = ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')
TIME_KEYS = ('y_in', 'sh_t', 'szh_t')


def make_batch(R, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, generator=g, device='cuda')
    s_dry, n_dry = 0.2 * rn(R, L), 0.1 * rn(R, L)

    def images(dry, taps, gain):
        h = gain * rn(R, K, taps) * torch.exp(-torch.arange(taps, device='cuda') / 12.0)
        h[..., 0] += 0.8
        out = torch.zeros((R, K, L), device='cuda')
        for t in range(taps):
            out[..., t:] += h[..., t:t + 1] * dry[:, None, :L - t]
        return out

    s_in, n_in = images(s_dry, 40, 0.3), images(n_dry, 30, 0.2)
    d = dict(s_in=s_in, n_in=n_in, sf_t=0.9 * s_in + 0.002 * rn(R, K, L), nf_t=0.3 * n_in, szf_t=0.8 * s_in + 0.004 * rn(R, K, L), nzf_t=0.6 * n_in,
             s_dry=s_dry, n_dry=n_dry)
    d['y_in'] = d['s_in'] + d['n_in']
    d['sh_t'] = d['sf_t'] + d['nf_t']
    d['szh_t'] = d['szf_t'] + d['nzf_t']
    return {k: v.contiguous() for k, v in d.items()}


def timed(fn, reps):
    fn()                                                                      # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, {'s_median': float(np.median(ts)), 's_min': float(np.min(ts)), 's_max': float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--flen', type=int, default=512)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    R = args.rooms
    sig = make_batch(R)
    lengths = np.random.default_rng(1).integers(5 * FS, 10 * FS + 1, R)
    for r in range(R):                                                        # nothing past a room's clip may matter
        for v in sig.values():
            v[r, ..., int(lengths[r]):] = float('nan')
    snrs = np.zeros((R, K))
    report = {'rooms': R, 'nodes': K, 'L': L, 'fs': FS, 'flen': args.flen, 'reps': args.reps, 'lengths_min': int(lengths.min()),
              'lengths_max': int(lengths.max())}

    def to_host(r):
        return {k: v[r, ..., :int(lengths[r])].cpu().numpy() for k, v in sig.items()}

    _, report['d2h_of_every_room'] = timed(lambda: [to_host(r) for r in range(R)], args.reps)
    for name, times, stoi in (('levels', False, False), ('bss', True, False), ('bss_stoi', True, True)):
        extra = (lambda s: {k: s[k] for k in TIME_KEYS}) if times else (lambda s: {})

        def batch():
            return rio.batch_results(*(sig[k] for k in ROOM_KEYS), snrs, s_dry=sig['s_dry'], n_dry=sig['n_dry'], fs=FS, bss_flen=args.flen,
                                     stoi=stoi, lengths=lengths, **extra(sig))

        def loop():
            out = []
            for r in range(R):
                h = to_host(r)
                out.append(rio.room_results(*(h[k] for k in ROOM_KEYS), snrs[r], s_dry=h['s_dry'], n_dry=h['n_dry'], fs=FS, bss_flen=args.flen,
                                            stoi=stoi, **extra(h)))
            return out

        (res, resz), tb = timed(batch, args.reps)
        rooms, tl = timed(loop, args.reps)
        same = all(np.array_equal(np.asarray(got[key])[r], np.asarray(want[key]), equal_nan=True)
                   for r in range(R) for got, want in ((res, rooms[r][0]), (resz, rooms[r][1])) for key in got)
        report[name] = {'batch_results': tb, 'room_results_loop': tl, 'loop_over_batch': tl['s_median'] / tb['s_median'], 'same_bits': bool(same)}
        print(json.dumps({name: report[name]}), flush=True)
    print(json.dumps(report), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(report, open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
