#!/usr/bin/env python3
"""Golden fixture for seg_snr, reverb_ratios, ci_wp and bar_data, produced by RUNNING THE REFERENCE'S OWN metrics.py / misc_utils.py.

    python -B tests/golden/make_golden_levels.py <directory that holds the reference's disco_theque package>

A scratch copy of disco_theque is imported, in the manner of make_golden_metrics.py.  seg_snr imports two helpers at call time that the
reference does not ship; stand-ins are placed in sys.modules -- the ONLY substituted pieces:
    disco_theque.sigproc_utils.sliding_window(x, win_len, win_hop, axis) = sliding_window_view(x, win_len)[::win_hop]
    disco_theque.db_utils.frame_vad(vad, win_len, win_hop)               = vad[::win_hop]
(the second is the decimation the reference itself applies to a per-sample VAD for its 'ivad' masks, tango.py:219-220).  Everything else --
the variances, the floor, the clip, the weighted mean, argmax, the two np.convolve calls, nanstd, the binning -- is the reference's code.
Every input is a float64 copy of a float32-representable array, so the reference's numbers are float64 arithmetic on exactly what the
kernels read.  Where the reference cannot answer (no whole window: sliding_window_view raises) the stored value is NaN, which is what
disco_amd.metrics.seg_snr defines there.  Writes tests/golden/levels_ref.npz: arrays only.

The case tables below are imported by tests/segsnr_checks.py and tests/reverb_checks.py, so that the generator and the checks cannot
disagree about what a row of the fixture is.
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- seg_snr -------------------------------------------------------------------------------------------------------------------
SEG_LEN = 6300                                                   # start 300 + the longest span
SEG_WINDOWS = ((512, 256), (400, 160), (512, 512), (7, 3), (1, 1))
VAD_NONE, VAD_BINARY, VAD_FRACTION, VAD_ZERO = -1, 0, 1, 2       # rows of seg_vad


def seg_signals():
    """-> s, n (3, SEG_LEN) float32, vad (3, SEG_LEN) float32.  Row 0: coloured noise.  Row 1: stretches where s is exactly zero, where n
    is, and where both are (aligned to windows of 512 / 256 and of 7 / 3 from sample 0).  Row 2: a large constant offset on one stretch."""
    rng = np.random.default_rng(41)
    s = np.stack([np.convolve(rng.standard_normal(SEG_LEN + 2), [1, 0.6, 0.3])[2:SEG_LEN + 2] for _ in range(3)])
    n = np.stack([0.3 * np.convolve(rng.standard_normal(SEG_LEN + 1), [1, -0.4])[1:SEG_LEN + 1] for _ in range(3)])
    s[0] *= np.repeat(10 ** (rng.uniform(-2.5, 1.5, SEG_LEN // 150)), 150)          # levels that reach both clip bounds
    s[1, 512:1280] = 0.0
    n[1, 2048:2816] = 0.0
    s[1, 3584:4352] = 0.0
    n[1, 3584:4352] = 0.0
    s[2, 1000:2100] += 1000.0
    n[2, 3000:3700] -= 4096.0
    vad = np.stack([np.repeat(rng.integers(0, 2, SEG_LEN // 100), 100).astype(np.float64), rng.uniform(0, 1, SEG_LEN), np.zeros(SEG_LEN)])
    return s.astype(np.float32), n.astype(np.float32), vad.astype(np.float32)


def seg_cases():
    """-> int array (n_case, 6): row of the signals, start, stop, win_len, win_hop, row of seg_vad (VAD_NONE: no VAD)."""
    c = []
    for w, h in SEG_WINDOWS:
        for L in (w - 1, w, w + h - 1, w + h, 6000):
            c.append((0, 0, L, w, h, VAD_NONE))
    for row in (1, 2):
        for w, h in ((512, 256), (7, 3), (1, 1)):
            c.append((row, 0, 6000, w, h, VAD_NONE))
    for row in (0, 1):
        for v in (VAD_BINARY, VAD_FRACTION, VAD_ZERO):
            c.append((row, 0, 6000, 512, 256, v))
            c.append((row, 0, 1501, 400, 160, v))
    for row, stop in ((0, 6300), (1, 5321), (2, 4000), (0, 811), (1, 812)):
        c.append((row, 300, stop, 512, 256, VAD_NONE))
        c.append((row, 300, stop, 512, 256, VAD_FRACTION))
    return np.array(c, dtype=np.int64)


# ---- reverb_ratios -------------------------------------------------------------------------------------------------------------
FS = 16000
REVERB_SHAPES = ((1500, 700, 5, 3), (1500, 1024, 5, 3), (1500, 1300, 5, 3), (512, 513, 5, 3), (1, 700, 5, 3), (600, 8192, 1, 3))   # Ld, rir_len, n_sig, n_ch
# where the split falls; the peak index and reverb_start (ms; n_d = int(1e-3 reverb_start fs) = 0 / 40 / 320) that put it there
SPLIT_KINDS = ('one', 'inside_first', 'at_512', 'at_1024', 'inside_last', 'last_tap')


def split_plan(kind, rir_len):
    """-> (peak index, reverb_start in ms, split) or None where the response is too short for the kind."""
    P = (rir_len + 511) // 512
    plan = {'one': (1, 0.0), 'inside_first': (30, 20.0), 'at_512': (192, 20.0), 'at_1024': (984, 2.5),
            'inside_last': ((P - 1) * 512 + (rir_len - (P - 1) * 512) // 2 - 40, 2.5), 'last_tap': (rir_len - 41, 2.5)}[kind]
    peak, rs = plan
    split = peak + int(1e-3 * rs * FS)
    if peak < 0 or not 0 < split < rir_len:
        return None
    return peak, rs, split


def reverb_inputs(shape_index):
    """-> x (n_sig, Ld), rir (n_sig, n_ch, rir_len) float32, reverb_start (n_sig, n_ch) float64, kinds (n_sig, n_ch) indices of SPLIT_KINDS.
    Responses: a unit peak on an exponentially decaying noise floor.  Special rows of shape 2 (1500, 1300):
      (0, 0)  the tail's energy sits in the output blocks past the end of the dry signal: tap rir_len - 1 and the last dry sample are large;
      (1, 1)  a direct path 40 dB above the tail."""
    Ld, Lh, n_sig, n_ch = REVERB_SHAPES[shape_index]
    rng = np.random.default_rng(100 + shape_index)
    x = np.convolve(rng.standard_normal((n_sig * (Ld + 1),)), [1, 0.7])[1:].reshape(n_sig, Ld + 1)[:, :Ld].copy()
    rir = np.zeros((n_sig, n_ch, Lh))
    rs = np.zeros((n_sig, n_ch))
    kinds = np.zeros((n_sig, n_ch), dtype=np.int64)
    t = np.arange(Lh)
    usable = [k for k in range(len(SPLIT_KINDS)) if split_plan(SPLIT_KINDS[k], Lh) is not None]
    for i in range(n_sig):
        for c in range(n_ch):
            k = usable[(i * n_ch + c) % len(usable)]
            peak, rs[i, c], split = split_plan(SPLIT_KINDS[k], Lh)
            kinds[i, c] = k
            h = 0.2 * rng.standard_normal(Lh) * np.exp(-t / (0.25 * Lh + 40.0))
            h = np.clip(h, -0.9, 0.9)
            h[peak] = 1.0
            if shape_index == 2 and (i, c) == (1, 1):
                h[split:] *= 0.01 * np.sqrt(np.sum(h[:split] ** 2) / np.sum(h[split:] ** 2))
            rir[i, c] = h
    if shape_index == 2:
        rir[0, 0, Lh - 1] = 0.95
        rir[0, 0, Lh - 300:Lh - 1] *= 1e-3
        x[0, Ld - 1] = 40.0
    return x.astype(np.float32), rir.astype(np.float32), rs, kinds


# ---- ci_wp / bar_data ----------------------------------------------------------------------------------------------------------
def table_inputs():
    rng = np.random.default_rng(7)
    ci_x = rng.standard_normal((9, 4))
    ci_x[2, 1] = ci_x[5, 1] = np.nan
    ci_x[:, 3] = np.nan
    edges = np.array([-5.0, 0.0, 5.0, 10.0, 15.0])
    bx = rng.uniform(-9.0, 10.0, 40)
    bx[bx > 5.0] += 5.0                                              # nothing lands in (5, 10]: an empty bin
    by = rng.standard_normal(40) * 3 + 8
    by[3] = np.nan
    return ci_x, edges, bx, by


def main():
    from numpy.lib.stride_tricks import sliding_window_view
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('DISCO_REFERENCE')
    if not ref_dir or not os.path.isdir(os.path.join(ref_dir, 'disco_theque')):
        sys.exit(__doc__)
    sys.dont_write_bytecode = True
    scratch = tempfile.mkdtemp(prefix='disco_ref_')
    shutil.copytree(os.path.join(ref_dir, 'disco_theque'), os.path.join(scratch, 'disco_theque'))
    sys.path.insert(0, scratch)
    sp = types.ModuleType('disco_theque.sigproc_utils')
    sp.sliding_window = lambda x, win_len, win_hop, axis=-1: sliding_window_view(x, win_len)[::win_hop]
    db = types.ModuleType('disco_theque.db_utils')
    db.frame_vad = lambda vad, win_len, win_hop: vad[::win_hop]
    sys.modules['disco_theque.sigproc_utils'] = sp
    sys.modules['disco_theque.db_utils'] = db
    from disco_theque import metrics as ref                      # the reference's own module
    from disco_theque import misc_utils as ref_misc

    out = {}
    s, n, vad = seg_signals()
    cases = seg_cases()
    seg_ref = np.full(len(cases), np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        for q, (row, start, stop, w, h, v) in enumerate(cases):
            if stop - start < w:
                continue                                         # no whole window: the reference cannot answer
            a, b = s[row, start:stop].astype(np.float64), n[row, start:stop].astype(np.float64)
            g = None if v == VAD_NONE else vad[v, start:stop].astype(np.float64)
            seg_ref[q] = ref.seg_snr(a, b, int(w), int(h), vad=g)
    out.update(seg_s=s, seg_n=n, seg_vad=vad, seg_cases=cases, seg_ref=seg_ref)

    for k in range(len(REVERB_SHAPES)):
        x, rir, rs, kinds = reverb_inputs(k)
        drr, srr = np.zeros(rs.shape), np.zeros(rs.shape)
        for i in range(rir.shape[0]):
            for c in range(rir.shape[1]):
                drr[i, c], srr[i, c] = ref.reverb_ratios(x[i].astype(np.float64), rir[i, c].astype(np.float64), reverb_start=rs[i, c], fs=FS)
        out.update({f'rev{k}_x': x, f'rev{k}_rir': rir, f'rev{k}_start': rs, f'rev{k}_kind': kinds, f'rev{k}_drr': drr, f'rev{k}_srr': srr})

    ci_x, edges, bx, by = table_inputs()
    import warnings
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        means, cis = ref_misc.bar_data(edges, bx, by)
        out.update(ci_x=ci_x, ci_axis0=ref.ci_wp(ci_x), ci_axis1=ref.ci_wp(ci_x, axis=1), bar_edges=edges, bar_x=bx, bar_y=by,
                   bar_means=means, bar_cis=cis)
    np.savez_compressed(os.path.join(HERE, 'levels_ref.npz'), **out)
    shutil.rmtree(scratch, ignore_errors=True)
    print('wrote levels_ref.npz', os.path.getsize(os.path.join(HERE, 'levels_ref.npz')), 'bytes')
    print('seg_ref', np.round(seg_ref, 3))
    for k in range(len(REVERB_SHAPES)):
        print(REVERB_SHAPES[k], 'drr', np.round(out[f'rev{k}_drr'], 1).tolist(), 'srr', np.round(out[f'rev{k}_srr'], 1).tolist())


if __name__ == '__main__':
    main()
