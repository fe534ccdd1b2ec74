"""The reference side of tests/sources_checks.py alone (no GPU, no emulator): the conditions under which its comparisons mean something.
  - next_pow_2 in integers is the reference's float expression at every 2^k - 1, 2^k, 2^k + 1 up to 2^22 + 1;
  - the three-line restatement of noise_from_signal reproduces the fixture's reference outputs exactly, from the stored phases;
  - the float32 CPU transform that sets the noise bar is itself near the float64 statement (a bar of 4 x a sound yardstick);
  - every levelled target of the fixture keeps min |x2 - thr_| / thr_ >= 2e-4 before and after the scaling, its voiced variance is var_tar,
    and the three cases are the ones the checks rely on (one trimmed, one refused, each with a non-zero mean);
  - the NumPy statement of the affine pass wraps as np.roll does;
  - the lengths noise_from_signal cannot take are refused before anything touches a device, naming the limit;
  - the C ABI and the package declare the new surface, and the library holds no FFT it did not write."""
import os

import numpy as np
import pytest

import sources_checks as sc
from oracle import mwf_oracle as mo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_is_declared():
    from disco_amd import _lib, dataset_utils, math_utils, sigproc_utils
    from disco_amd.engine import Engine
    hdr = open(os.path.join(REPO, 'include', 'disco_hip.h')).read()
    for name, n_args in (('disco_noise_from_signal', 9), ('disco_affine_segment', 13)):
        assert name in _lib.PROTOTYPES and f'int {name}(' in hdr, name
        assert len(_lib.PROTOTYPES[name][1]) == n_args
    assert all(callable(getattr(dataset_utils, f)) for f in ('target_segments', 'noise_segments', 'ssn_segments'))
    assert set(('target_segments', 'noise_segments', 'ssn_segments')) <= set(dataset_utils.__all__)
    assert callable(sigproc_utils.noise_from_signal) and callable(math_utils.next_pow_2)
    assert callable(Engine.noise_from_signal) and callable(Engine.affine_segment)
    for f in ('api_sources.hip', 'k_sources.h'):
        assert os.path.exists(os.path.join(REPO, 'disco_amd', 'csrc', f))


def test_library_holds_no_foreign_fft():
    """No source of the library names a foreign FFT.  disco_amd/synth.py, the benchmark's scene synthesis, is the one file that did before
    the dry sources moved to the device (its torch.fft convolution is the alternative route to Engine.rir_convolve) and is not looked at."""
    pkg = os.path.join(REPO, 'disco_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.h', '.hip')) and f != 'synth.py':
                text = open(os.path.join(root, f), errors='replace').read()
                for word in ('torch.fft', 'rocfft', 'hipfft'):
                    assert word not in text, (f, word)


def test_next_pow_2_is_the_reference():
    from disco_amd.math_utils import next_pow_2
    for k in range(0, 23):
        for x in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            if x >= 1:
                assert next_pow_2(x) == sc.next_pow_2_reference(x), x
    assert next_pow_2(1) == 1 and next_pow_2(513) == 1024 and next_pow_2(2 ** 22) == 2 ** 22 and next_pow_2(2 ** 22 + 1) == 2 ** 23
    with pytest.raises(ValueError):
        next_pow_2(0)


def test_restatement_is_the_reference():
    fx = sc.fixture()
    assert int(fx['n_noise']) == 3
    lengths = []
    for i in range(int(fx['n_noise'])):
        x, u, y = fx[f'noise_x{i}'], fx[f'noise_u{i}'], fx[f'noise_y{i}']
        assert x.dtype == np.float32 and u.dtype == np.float64 and y.dtype == np.float64
        n_fft = 2 * (len(u) - 1)
        assert n_fft == sc.next_pow_2_reference(len(x)) and u.min() >= 0 and u.max() < 1
        assert np.array_equal(sc.restate(x, u, n_fft), y), i                 # difference 0.0
        np.random.seed(int(fx['noise_seed'][i]))
        assert np.array_equal(np.random.random(len(u)), u), 'the stored phases are the seeded draw'
        assert 0.05 < np.std(x) < 0.2
        lengths.append(len(x))
    assert lengths == [1500, 5000, 4096] and sc.next_pow_2_reference(4096) == 4096


def test_the_yardstick_is_sound():
    """The float32 CPU transform stays within a small multiple of float32's precision of the float64 statement."""
    for p in (10, 13, 18):
        n = 1 << p
        x, u = sc.coloured(n, p), sc.phases(n // 2 + 1, p + 1)
        rel, peak = sc.figures(sc.torch_route(x, u, n), sc.restate(x, u, n))
        print(f'torch float32 route at 2^{p}: rel L2 {rel:.3e}, max / rms {peak:.3e}')
        assert 1e-8 < rel < 2e-6 and 1e-8 < peak < 5e-5, (p, rel, peak)


def test_target_fixture_conditions():
    fx = sc.fixture()
    fs, var_tar = int(fx['fs']), float(fx['var_tar'])
    lo, hi = (float(v) for v in fx['duration_range'])
    lens = fx['target_len']
    assert lens.max() <= 20000 and (lens > int(hi * fs)).sum() == 1 and (lens / fs < lo).sum() == 1
    assert np.array_equal(fx['target_ok'], lens / fs >= lo)
    for i, L in enumerate(lens):
        x = fx['target_x'][i, :L].astype(np.float64)
        assert abs(np.mean(x)) > 5e-3, 'a non-zero mean'
        trimmed = x[:int(hi * fs)]
        assert fx['target_duration'][i] == len(trimmed) / fs + 1
        if not fx['target_ok'][i]:
            assert fx['target_out_len'][i] == 0 and not fx['target_signal'][i].any()
            continue
        n_out = int(fx['target_out_len'][i])
        assert n_out == fs + len(trimmed)
        s, v = fx['target_signal'][i, :n_out].astype(np.float64), fx['target_vad'][i, :n_out]
        margins = (sc.vad_margin(trimmed - np.mean(trimmed)), sc.vad_margin(s[fs:]))
        print('target', i, 'VAD margins before / after the scaling', margins)
        assert min(margins) >= 2e-4, margins
        assert not s[:fs].any() and not v[:fs].any() and 0 < v.mean() < 1
        # the reference's own arithmetic again, through the oracle's vad_oracle_batch
        d = trimmed - np.mean(trimmed)
        v1 = mo.vad_oracle_batch(d, thr=0.001)
        scaled = d * np.sqrt(var_tar / np.var(d[v1 == 1]))
        assert np.abs(scaled - s[fs:]).max() <= 1e-7 * np.abs(scaled).max()      # the fixture stores float32
        assert np.array_equal(mo.vad_oracle_batch(scaled, thr=0.001), v[fs:])
        assert abs(np.var(scaled[v1 == 1]) / var_tar - 1) < 1e-12


def test_affine_statement_wraps_like_roll():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 50)).astype(np.float32)
    for start in (0, 1, 17, 49):
        got = sc.affine_reference(x, None, np.array([start]), 30, 0.0, 1.0, 0, 30)
        assert np.array_equal(got[0], np.roll(x[0], 50 - start)[:30]), start
    periodic = sc.affine_reference(x, np.array([7]), np.array([6]), 10, 0.0, 1.0, 2, 14)
    assert np.array_equal(periodic[0, 2:12], x[0, (6 + np.arange(10)) % 7]) and not periodic[0, :2].any() and not periodic[0, 12:].any()


def test_lengths_outside_the_transform_are_refused_on_the_host():
    from disco_amd.sigproc_utils import noise_from_signal
    for L, stop in ((512, None), (2000, np.array([2000, 512])), ((1 << 22) + 1, None)):
        x = np.zeros((2, L), np.float32)
        with pytest.raises(ValueError, match='513 to 4194304'):
            noise_from_signal(x, stop=stop)
