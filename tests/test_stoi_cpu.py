"""The float64 STOI yardstick of tests/stoi_checks.py on its own (no library, no GPU): against its whole-array form, the band table and
tap counts, the polyphase statement of the resampler against scipy, closed forms, monotony in SNR, and the float32 floor behind
TOL_STOI."""
import numpy as np
import pytest
import scipy.signal

import stoi_checks as sc


def test_yardstick_against_its_vectorised_form():
    worst = 0.0
    for fs, n in sc.CASES:
        for snr in sc.SNRS:
            a, b = sc.yard_of(1, n, fs, snr), sc.yard_of(1, n, fs, snr, vectorised=True)
            assert (a.status, a.n_kept, a.T, a.kept) == (b.status, b.n_kept, b.T, b.kept) and a.margin == b.margin
            worst = max(worst, abs(a.d - b.d))
    print(f'loops against whole arrays: worst |diff| = {worst:.3g}')
    assert worst < 1e-13


def test_band_table_and_tap_counts():
    lo, hi = sc.band_table()
    assert lo.tolist() == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert (hi - lo).tolist() == [2, 2, 3, 3, 5, 5, 7, 9, 12, 14, 18, 22, 29, 36, 45] and hi[-1] - 1 == 218
    assert hi[:-1].tolist() == lo[1:].tolist()           # what csrc/k_stoi.h relies on: a band ends where the next begins
    for fs, taps, pq in ((16000, 581, (5, 8)), (8000, 365, (5, 4)), (48000, 1741, (5, 24))):
        p, q, h = sc.resample_taps(fs)
        assert (p, q) == pq and len(h) == taps and abs(np.sum(h) - 1) < 1e-15
    w = sc.window()
    assert len(w) == 256 and np.allclose(w, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1, 257) / 257), rtol=0, atol=1e-15)


def test_engine_taps_are_the_yardsticks():
    from disco_amd.engine import stoi_resample_taps
    for fs in (16000, 8000, 48000, 44100):
        p, q, h = stoi_resample_taps(fs)
        p2, q2, h2 = sc.resample_taps(fs)
        assert (p, q) == (p2, q2) and np.array_equal(h, h2)
    assert stoi_resample_taps(10000)[:2] == (1, 1)


@pytest.mark.parametrize('fs,n', [(16000, 1203), (16000, 1200), (8000, 901), (48000, 4805)])
def test_polyphase_formula_equals_scipy(fs, n):
    x = np.random.default_rng(fs + n).standard_normal(n)
    p, q, h = sc.resample_taps(fs)
    want = scipy.signal.resample_poly(x, p, q, window=h)
    got = sc.polyphase(x, fs)
    assert got.shape == want.shape == (-(-n * p // q),)
    err = float(np.max(np.abs(got - want)))
    print(f'fs {fs} n {n}: polyphase against resample_poly, worst |diff| = {err:.3g}')
    assert err < 1e-14


def test_closed_forms():
    x, _ = sc.make_pair(1, 16000, 16000, 5.0)
    x = x.astype(np.float64)
    for y in (x, 3 * x, -x):
        assert abs(sc.stoi_yardstick(x, y, 16000).d - 1) < 1e-12


def test_d_falls_with_snr():
    for seed in sc.SEEDS:
        d = [sc.yard_of(seed, 16000, 16000, snr).d for snr in sc.SNRS]
        assert d[0] > d[1] > d[2], d


def test_compared_cases_meet_the_precondition():
    for fs, n, seed, snr in sc.compared_cases():
        sc.assert_precondition(sc.yard_of(seed, n, fs, snr), (fs, n, seed, snr))


def test_float32_floor():
    """Worst |float32-staged - float64| over the committed case list: the number behind TOL_STOI."""
    worst, margins, ds = 0.0, [], []
    for fs, n, seed, snr in sc.compared_cases():
        x, y = sc.make_pair(seed, n, fs, snr)
        a, b = sc.yard_of(seed, n, fs, snr), sc.stoi_f32_staged(x, y, fs)
        assert a.kept == b.kept
        worst = max(worst, abs(a.d - b.d))
        margins.append(a.margin)
        ds.append(a.d)
    tol = 16 * worst
    digit = 10 ** np.floor(np.log10(tol))
    rule = min(np.ceil(tol / digit) * digit, 1e-6)
    print(f'float32 floor over {len(ds)} cases: {worst:.3g}; 16 x = {tol:.3g} -> {rule:.0e}; margins {min(margins):.3g} .. {max(margins):.3g} dB; '
          f'd {min(ds):.3f} .. {max(ds):.3f}')
    assert worst <= sc.FLOOR_MEASURED * 1.0001, (worst, sc.FLOOR_MEASURED)       # the committed figure is the measured one
    assert np.isclose(sc.TOL_STOI, min(np.ceil(16 * sc.FLOOR_MEASURED / digit) * digit, 1e-6), rtol=1e-9), (sc.TOL_STOI, rule)
