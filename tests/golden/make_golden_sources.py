#!/usr/bin/env python3
"""Golden fixture for the dry sources (tests/sources_checks.py), produced by RUNNING THE REFERENCE'S OWN CODE:
    disco_theque/sigproc_utils.py                   noise_from_signal (257-279), vad_oracle_batch (12-55)
    disco_theque/math_utils.py                      next_pow_2 (155-165)
    disco_theque/dataset_utils/signal_setups.py     SpeechAndNoiseSetup.get_target_segment (42-73)
The function sources are taken with `ast` (the modules import soundfile and python-acoustics, both absent); the method is exec'd as a plain
function of `self`.  `np.int`, which NumPy >= 1.24 removed, is restored by the proxy of make_golden_ivad.py; `sf.read` is an in-memory
stand-in that hands out a float64 copy of a named array.  noise_from_signal draws its phases from NumPy's global generator: it is seeded,
and the same seed replayed gives the phases that are stored beside the output.
Inputs (float32):
    noise    coloured noise of amplitude ~ 0.1 at L = 1500, 5000 (n_fft 2048, 8192) and L = 4096 (L == n_fft)
    targets  three speech-like burst signals with a non-zero mean at fs = 16 kHz, duration_range (0.5, 1.0) s: 20 000 samples (longer than
             max_duration: trimmed to 16 000), 12 000, and 6 000 (shorter than min_duration: the reference returns None)
The seed is advanced until every levelled target keeps min |x2 - thr_| / thr_ >= 2e-4 both before and after the scaling, so that the
sample-exact VAD comparison is meaningful.  The fixture holds arrays only.
Runs only in the build container.      python -B tests/golden/make_golden_sources.py
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
REF = '/root/reference'
FS, VAR_TAR, DURATION_RANGE = 16000, 1e-3, (0.5, 1.0)
NOISE_LENGTHS = (1500, 5000, 4096)
NOISE_SEEDS = (11, 12, 13)
TARGET_LENGTHS = (20000, 12000, 6000)


def vad_margin(x):
    """min |x2 - thr_| / thr_ with the reference's own arithmetic (sigproc_utils.py:42-45)."""
    d = x - np.mean(x)
    x2 = abs(d ** 2)
    thr_ = 0.001 * np.quantile(x2, 0.99)
    return float(np.min(np.abs(x2 - thr_)) / thr_)


def _function(path, name, cls=None):
    src = open(path).read()
    body = ast.parse(src).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    return textwrap.dedent('\n'.join(src.splitlines()[node.lineno - 1:node.end_lineno]))


def coloured(rng, L):
    x = scipy.signal.lfilter([1.0, -0.5], [1.0, -1.3, 0.6], rng.standard_normal(L))
    return (0.1 * x / np.std(x)).astype(np.float32)


def bursts(rng, L, offset):
    x = scipy.signal.lfilter([1.0, -0.6], [1.0, -1.2, 0.52], rng.standard_normal(L))
    env = np.zeros(L)
    t = int(rng.integers(200, 900))
    while t < L:
        on, off = int(rng.integers(900, 2500)), int(rng.integers(400, 1200))
        env[t:t + on] = 10.0 ** rng.uniform(-0.5, 0.0)
        t += on + off
    return (0.05 * x * env + offset).astype(np.float32)


def main():
    from make_golden_ivad import _NumpyWithInt
    npx = _NumpyWithInt()
    ns = {'np': npx}
    exec(_function(os.path.join(REF, 'disco_theque/math_utils.py'), 'next_pow_2'), ns)
    exec(_function(os.path.join(REF, 'disco_theque/sigproc_utils.py'), 'vad_oracle_batch'), ns)
    exec(_function(os.path.join(REF, 'disco_theque/sigproc_utils.py'), 'noise_from_signal'), ns)
    files = {}
    ns['sf'] = types.SimpleNamespace(read=lambda name: (files[name].astype(np.float64).copy(), FS))
    exec(_function(os.path.join(REF, 'disco_theque/dataset_utils/signal_setups.py'), 'get_target_segment', cls='SpeechAndNoiseSetup'), ns)
    noise_from_signal, next_pow_2, get_target_segment = ns['noise_from_signal'], ns['next_pow_2'], ns['get_target_segment']

    out = {'fs': np.array(FS), 'var_tar': np.array(VAR_TAR), 'duration_range': np.array(DURATION_RANGE), 'n_noise': np.array(len(NOISE_LENGTHS)),
           'n_target': np.array(len(TARGET_LENGTHS)), 'noise_seed': np.array(NOISE_SEEDS)}
    # ---- noise_from_signal under a seed; the same seed replayed gives its phases
    rng = np.random.default_rng(777)
    for i, (L, seed) in enumerate(zip(NOISE_LENGTHS, NOISE_SEEDS)):
        x = coloured(rng, L)
        np.random.seed(seed)
        y = noise_from_signal(x.astype(np.float64))           # what sf.read hands over: float64
        np.random.seed(seed)
        u = np.random.random(next_pow_2(L) // 2 + 1)
        X = np.fft.rfft(x.astype(np.float64), next_pow_2(L))
        restated = np.fft.irfft(np.abs(X) * np.exp(2j * np.pi * u), next_pow_2(L))[:L]
        assert np.array_equal(restated, y), 'the three-line restatement is not the reference'
        out[f'noise_x{i}'], out[f'noise_u{i}'], out[f'noise_y{i}'] = x, u, y
    # ---- get_target_segment
    seed = 4100
    while True:
        rng = np.random.default_rng(seed)
        sigs = [bursts(rng, L, off) for L, off in zip(TARGET_LENGTHS, (0.01, -0.02, 0.015))]
        res, margins = [], []
        for i, x in enumerate(sigs):
            files[f'target{i}'] = x
            me = types.SimpleNamespace(duration_range=DURATION_RANGE, var_tar=VAR_TAR, target_duration=None)
            s, v, fs = get_target_segment(me, f'target{i}')
            res.append((s, v, me.target_duration))
            if s is not None:
                trimmed = x.astype(np.float64)[:int(DURATION_RANGE[1] * FS)]
                margins += [vad_margin(trimmed - np.mean(trimmed)), vad_margin(s[FS:])]
        if min(margins) >= 2e-4:
            break
        seed += 1
    Lmax = max(len(s) for s, _, _ in res if s is not None)
    sig, vad = np.zeros((len(sigs), Lmax), np.float32), np.zeros((len(sigs), Lmax), np.uint8)
    raw = np.zeros((len(sigs), max(TARGET_LENGTHS)), np.float32)
    for i, (x, (s, v, dur)) in enumerate(zip(sigs, res)):
        raw[i, :len(x)] = x
        if s is not None:
            sig[i, :len(s)], vad[i, :len(v)] = s, v
    out.update(target_x=raw, target_len=np.array(TARGET_LENGTHS), target_signal=sig, target_vad=vad, target_seed=np.array(seed),
               target_ok=np.array([s is not None for s, _, _ in res]), target_out_len=np.array([0 if s is None else len(s) for s, _, _ in res]),
               target_duration=np.array([d for _, _, d in res]))
    voiced = [float(np.var(s[v == 1])) for s, v, _ in res if s is not None]
    path = os.path.join(HERE, 'sources_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote sources_ref.npz', os.path.getsize(path), 'bytes; target seed', seed, 'VAD margins', margins, 'ok', out['target_ok'],
          'voiced variance after the second VAD', voiced, 'active', [float(v.mean()) for _, v, _ in res if v is not None])


if __name__ == '__main__':
    main()
