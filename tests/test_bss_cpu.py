"""The two float64 yardsticks of the BSS-eval tests (tests/bss_checks.py: dense_oracle, gram_oracle) against each other, without any
kernel: the delayed-reference matrix with np.linalg.lstsq and residual signals, and the lag-correlation / Cholesky route the kernels
follow.  They share nothing but the definition, so their agreement is what the kernels' tolerance (bss_checks.TOL_DB) is argued from."""
import numpy as np
import pytest

import bss_checks as bc


@pytest.mark.parametrize('kind', bc.SPECTRA)
def test_dense_and_gram_routes_agree(kind):
    """L = 6000, two references with 600 samples of silence each, flen 512: cond(G) <= 1e7, agreement to 1e-9 dB (measured: 2e-12)."""
    refs, ests = bc.make_case(kind, 6000, 2)
    cond = bc.cond_gram(refs, 512)
    d, g = bc.dense_oracle(refs, ests[0], 0, 512), bc.gram_oracle(refs, ests[0], 0, 512)
    err = max(abs(a - b) for a, b in zip(d, g))
    print(f'{kind}: cond(G) = {cond:.3g}, dense {d}, gram {g}, |diff| = {err:.3g} dB')
    assert cond <= 1e7
    assert all(5 < v < 40 for v in d)
    assert err < 1e-9


@pytest.mark.parametrize('flen', (64, 256))
def test_routes_agree_at_the_conditioning_of_real_recordings(flen):
    """Order-8 low-pass references with a white floor of 1e-5 (16-bit audio sits near 3e-5): cond(G) <= 1e11, agreement to 1e-8 dB."""
    refs, ests = bc.make_case('floor1e-5', 5000, 2)
    cond = bc.cond_gram(refs, flen)
    worst = 0.0
    for j in range(2):
        d, g = bc.dense_oracle(refs, ests[j], j, flen), bc.gram_oracle(refs, ests[j], j, flen)
        worst = max(worst, max(abs(a - b) for a, b in zip(d, g)))
        print(f'flen {flen} source {j}: cond(G) = {cond:.3g}, dense {d}, gram {g}')
    assert 1e8 < cond <= 1e11
    assert worst < 1e-8, worst


def test_three_references_second_target():
    refs, ests = bc.make_case('fir', 3000, 3)
    d, g = bc.dense_oracle(refs, ests[1], 1, 64), bc.gram_oracle(refs, ests[1], 1, 64)
    assert max(abs(a - b) for a, b in zip(d, g)) < 1e-9


def test_lag_correlation_oracle_against_numpy():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((2, 300))
    full = np.correlate(b, a, 'full')                                   # full[k] = sum_n b[n + k - (L - 1)] a[n]
    lags = range(-40, 41)
    assert np.allclose(bc.lag_corr_oracle(a, b, lags), [full[t + 299] for t in lags], rtol=0, atol=1e-12)


def test_host_arithmetic_of_the_figures():
    """disco_amd.metrics._figures: mir_eval's dB rules on the three energies (no kernel involved)."""
    from disco_amd import metrics as dm
    en = np.array([[4.0, 6.0, 10.0, 0.0],          # plain
                   [4.0, 4.0, 4.0, 0.0],           # nothing left over: +inf everywhere
                   [4.0, 3.999, 3.998, 0.0],       # differences below zero are clamped: +inf
                   [np.nan, np.nan, np.nan, 1.0]])
    sdr, sir, sar = dm._figures(en)
    assert np.allclose([sdr[0], sir[0], sar[0]], [10 * np.log10(4 / 6), 10 * np.log10(4 / 2), 10 * np.log10(6 / 4)], rtol=0, atol=1e-12)
    assert np.all(np.isinf([sdr[1], sir[1], sar[1], sdr[2], sir[2], sar[2]])) and np.all(np.isnan([sdr[3], sir[3], sar[3]]))
