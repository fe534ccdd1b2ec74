#!/usr/bin/env python3
"""Golden fixture for the steps between a reverberated source and a room (tests/roomsynth_checks.py), produced by RUNNING THE REFERENCE'S
OWN CODE:
    disco_theque/sigproc_utils.py                      vad_oracle_batch (12-55), fw_snr (120-190), increase_to_snr (194-224)
    dataset_generation/gen_disco/convolve_signals.py   snr_at_mics (170-213)
The function sources are taken with `ast` (the modules import soundfile, python-acoustics and pyroomacoustics, all absent).  `np.int`,
which NumPy >= 1.24 removed, is restored by the proxy of make_golden_ivad.py; `third_octave_filterbank` is the stand-in of
make_golden_metrics.py (oracle.metrics_oracle: the restated IEC 61260-1 band edges + scipy.signal.butter).  lin2db / db2lin are the
reference's math_utils.  Everything else is the reference's code.
Inputs (float32): R = 3 rooms, n_mic = 4 (K = 2, M = 2; ragged (2, 1) on the first three channels; (1, 1, 2) for the three-node case),
L = 8192 at 16 kHz; target images with a leading silence and bursts, coloured noise images, block VADs as in metrics_ref.npz.  The seed is
advanced until every target image keeps min |x2 - thr_| / thr_ >= 2e-4, so that the sample-exact VAD comparison is meaningful.
The fixture holds arrays only.  Runs only in the build container.      python -B tests/golden/make_golden_roomsynth.py
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
REF = '/root/reference'
FS, R, N_MIC, L = 16000, 3, 4, 8192
CASES = {'u': (2, 2), 'r': (2, 1), 't': (1, 1, 2)}            # uniform, ragged (first three channels), three nodes
SNR_OUT = (3.0, 0.0, 1.5)                                     # increase_to_snr: one target SNR per room; no band reaches fw_snr's clip bounds
SUB = 4                                                       # the scaled noises are kept at every 4th sample (one gain per signal)


def vad_margin(x):
    """min |x2 - thr_| / thr_ with the reference's own float32 arithmetic (sigproc_utils.py:42-45)."""
    d = x - np.mean(x)
    x2 = abs(d ** 2)
    thr_ = 0.001 * np.quantile(x2, 0.99)
    return float(np.min(np.abs(x2 - thr_)) / thr_)


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    tar = np.zeros((R, N_MIC, L))
    noi = np.zeros((R, N_MIC, L))
    # per-channel noise levels: room 0 gives node SNRs that are not monotonic over (1, 1, 2), so "all pairs" != "consecutive"
    noise_db = np.array([[-6.0, 0.0, -5.0, -5.5], [-2.0, -4.0, 1.0, -1.0], [0.0, -3.0, -6.0, -2.0]])
    for r in range(R):
        dry = scipy.signal.lfilter([1.0, -0.6], [1.0, -1.2, 0.52], rng.standard_normal(L))
        env = np.zeros(L)
        t = 900 + 100 * r                                       # leading silence
        while t < L:
            on, off = int(rng.integers(700, 1800)), int(rng.integers(300, 900))
            env[t:t + on] = 10.0 ** rng.uniform(-0.5, 0.0)
            t += on + off
        dry = 0.05 * dry * env
        base = np.convolve(rng.standard_normal(L), [1, -0.3, 0.1])[:L]
        for c in range(N_MIC):
            h = np.zeros(24)
            h[int(rng.integers(0, 6))] = 1.0
            h += 0.3 * rng.standard_normal(24) * np.exp(-np.arange(24) / 6.0)
            tar[r, c] = np.convolve(dry, h)[:L]
            g = np.zeros(16)
            g[int(rng.integers(0, 4))] = 1.0
            g += 0.2 * rng.standard_normal(16)
            noi[r, c] = 0.05 * 10 ** (noise_db[r, c] / 20) * np.convolve(base + 0.3 * rng.standard_normal(L), g)[:L]
    blk = lambda: np.repeat(rng.integers(0, 2, (R, L // 256)), 256, axis=1).astype(np.float32)
    return tar.astype(np.float32), noi.astype(np.float32), blk(), blk()


def _funcs(path, names):
    import ast
    src = open(path).read()
    return '\n\n'.join(ast.get_source_segment(src, node) for node in ast.parse(src).body
                       if isinstance(node, ast.FunctionDef) and node.name in names)


def main():
    from make_golden_ivad import _NumpyWithInt
    scratch = tempfile.mkdtemp(prefix='disco_ref_')
    shutil.copytree(os.path.join(REF, 'disco_theque'), os.path.join(scratch, 'disco_theque'))
    sys.path.insert(0, scratch)
    from disco_theque.math_utils import db2lin, lin2db
    from oracle import metrics_oracle as mo
    ns = {'np': _NumpyWithInt(), 'scipy': scipy, 'lin2db': lin2db, 'db2lin': db2lin, 'third_octave_filterbank': mo.third_octave_filterbank}
    exec(_funcs(os.path.join(scratch, 'disco_theque/sigproc_utils.py'), {'vad_oracle_batch', 'fw_snr', 'increase_to_snr'}), ns)
    exec(_funcs(os.path.join(REF, 'dataset_generation/gen_disco/convolve_signals.py'), {'snr_at_mics'}), ns)
    vad_oracle_batch, increase_to_snr, snr_at_mics = ns['vad_oracle_batch'], ns['increase_to_snr'], ns['snr_at_mics']

    seed = 20240
    while True:
        tar, noi, vad_a, vad_b = make_inputs(seed)
        margin = min(vad_margin(tar[r, c]) for r in range(R) for c in range(N_MIC))
        if margin >= 2e-4:
            break
        seed += 1
    out = {'fs': np.array(FS), 'seed': np.array(seed), 'tar': tar, 'noi': noi, 'vad_a': vad_a.astype(np.uint8), 'vad_b': vad_b.astype(np.uint8),
           'snr_out': np.array(SNR_OUT), 'sub': np.array(SUB)}
    # ---- the per-sample VAD of every target image (get_convolved_vads, convolve_signals.py:102-115), on the float32 signal itself
    image_vad = np.stack([[vad_oracle_batch(tar[r, c], thr=0.001) for c in range(N_MIC)] for r in range(R)])
    out['image_vad'] = image_vad.astype(np.uint8)
    # ---- snr_at_mics: with vad_s, and with vad_s and vad_n (one block VAD per room for all its channels)
    t64, n64 = tar.astype(np.float64), noi.astype(np.float64)
    for tag, mpn in CASES.items():
        nm = sum(mpn)
        for vtag in ('s', 'sn'):
            res = [snr_at_mics(t64[r, :nm], n64[r, :nm], np.array(mpn), FS, vad_s=image_vad[r, :nm],
                               vad_n=np.tile(vad_b[r], (nm, 1)) if vtag == 'sn' else None) for r in range(R)]
            out[f'snrs_{tag}_{vtag}'] = np.stack([v[0] for v in res])
            out[f'nodes_{tag}_{vtag}'] = np.stack([v[1] for v in res])
            out[f'delta_{tag}_{vtag}'] = np.array([v[2] for v in res])
    # ---- increase_to_snr on channel 0 of every room: both weight settings, with and without VADs
    for w in (False, True):
        for vads in (False, True):
            res = [increase_to_snr(t64[r, 0], n64[r, 0], SNR_OUT[r], vad_tar=vad_a[r] if vads else None, vad_noi=vad_b[r] if vads else None,
                                   weight=w, fs=FS) for r in range(R)]
            out[f'scaled_w{int(w)}_v{int(vads)}'] = np.stack(res)[:, ::SUB].astype(np.float32)
    path = os.path.join(HERE, 'roomsynth_ref.npz')
    np.savez_compressed(path, **out)
    shutil.rmtree(scratch, ignore_errors=True)
    print('wrote roomsynth_ref.npz', os.path.getsize(path), 'bytes; seed', seed, 'VAD margin', margin, 'active', float(image_vad.mean()))
    print('node SNRs', {k: np.round(v, 2).tolist() for k, v in out.items() if k.startswith('nodes_') and k.endswith('_s')})


if __name__ == '__main__':
    main()
