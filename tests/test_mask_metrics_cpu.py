"""The reference side of tests/mask_metric_checks.py alone (no kernel runs): the constant behind the oracle-mask bar is 4 x the worst
ratio of the float32 restatement, the inputs leave 'ibm' a band of at most 1e-3 of the bins, a NumPy restatement of the VAD kernel's
arithmetic agrees with the oracle on every frame of 1500 signals (so the reference alone admits the zero-frames bar), SciPy's own
distance from the long-double recurrence is what the module says it is, and the case lists hold the shapes they promise."""
import json
import os

import numpy as np
import pytest

import mask_metric_checks as mc
from oracle import mwf_oracle as mo


def test_oracle_mask_constant_is_four_times_the_float32_restatement():
    worst = mc.f32_restatement_ratio()
    print('mask_metrics_errors', json.dumps({'oracle_masks': {'f32_restatement_worst_ratio': round(worst, 4), 'C': mc.C_ORACLE}}))
    assert mc.C_ORACLE == pytest.approx(4 * worst, rel=2e-3)
    prof = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'mask_metrics_errors.json')))
    assert prof['oracle_masks']['C'] == mc.C_ORACLE
    assert prof['oracle_masks']['f32_restatement_worst_ratio'] == pytest.approx(worst, rel=2e-3)


def test_ibm_band_holds_at_most_1e3_of_the_bins():
    frac = mc.ibm_band_fraction()
    print('ibm band fraction', frac)
    assert frac <= 1e-3


def test_oracle_cases_hold_the_promised_shapes():
    cases = mc.oracle_cases()
    for n_fft in (512, 1024):
        for pad in ('reflect', 'constant'):
            mine = [c for c in cases if c[:2] == (n_fft, pad)]
            assert {c[2] for c in mine} == {15, 16, 17, 33, 65}
            assert any(c[3] == (c[2] - 1) * n_fft // 2 for c in mine) and all(1 + c[3] // (n_fft // 2) == c[2] for c in mine)
    assert {c[4] for c in cases} == {1, 3, 5}
    # wave items = n_sig x ceil(T / 16); some count is no multiple of the 4 waves of a block
    assert any((c[4] * -(-c[2] // 16)) % 4 for c in cases)
    cut = mc.oracle_cases(cut=True)
    assert set(cut) <= set(cases) and {c[0] for c in cut} == {512, 1024} and {c[1] for c in cut} == {'reflect', 'constant'}
    assert any(c[2] == 65 for c in cut)


def test_oracle_frames_are_the_oracles():
    """`_frames` (the norms behind delta, and the float32 restatement's input) frames as stft_oracle.stft does."""
    from oracle import stft_oracle as so
    x = np.random.default_rng(1).standard_normal((2, 3000)).astype(np.float32)
    for n_fft in (512, 1024):
        for pad in ('reflect', 'constant'):
            X = np.fft.rfft(mc._frames(x, n_fft, pad, np.float64), axis=-1)
            assert np.array_equal(np.swapaxes(X, -1, -2), so.stft(x, n_fft, n_fft // 2, pad, np.complex128))


def test_sensitivities_are_the_derivatives():
    """G against a finite difference of the mask in each magnitude."""
    rng = np.random.default_rng(2)
    aS, aN = rng.uniform(0.1, 3, 200), rng.uniform(0.1, 3, 200)
    h = 1e-6
    for kind in ('irm1', 'irm2', 'irm3'):
        p = int(kind[3])
        f = lambda s, n: (s / n) ** p / (1 + (s / n) ** p)
        fd = (np.abs(f(aS + h, aN) - f(aS - h, aN)) + np.abs(f(aS, aN + h) - f(aS, aN - h))) / (2 * h)
        assert np.allclose(mc._sens(aS, aN, None, kind), fd, rtol=1e-5)
    for kind in ('iam1', 'iam2'):
        p = int(kind[3])
        aY = rng.uniform(0.1, 3, 200)
        # |S + N| moves by up to 2 delta when both magnitudes move by delta
        fd = (np.abs((aS + h) ** p - (aS - h) ** p) / aY ** p + 2 * np.abs((aS / (aY + h)) ** p - (aS / (aY - h)) ** p)) / (2 * h)
        assert np.allclose(mc._sens(aS, None, aY, kind), fd, rtol=1e-5)


def test_sweep_and_special_inputs_reach_the_edges():
    S, N, mag = mc.sweep_inputs()
    assert mag.min() == 1e-38 and mag.max() == 1e38
    assert not np.isfinite(N).all() and np.isfinite(S).all()                  # |N| up to 1e40 leaves complex64
    with np.errstate(all='ignore'):
        r = np.abs(N.astype(np.complex128)) / np.abs(S.astype(np.complex128))
    ok = np.isfinite(r) & (np.abs(N) > 1e-37)
    assert r[ok].min() > 0.9e-2 and r[ok].max() < 1.1e2
    # the float32 reference is finite where the old sum of squares left float32: the sweep would have caught it
    inside = mc._in_float32(S, N, 'irm1')
    with np.errstate(all='ignore'):
        naive = np.sqrt(S.real ** 2 + S.imag ** 2)
    assert (inside & (mag >= 1e20) & np.isinf(naive)).any() and (inside & (mag <= 1e-24) & (naive == 0)).any()
    assert np.isfinite(mc.ref_mask32(S, N, 'irm1')[inside]).all()
    sp = mc.special_inputs()
    assert np.isnan(mc.ref_mask32(*sp['both 0'], 'iam1')).all() and np.isinf(mc.ref_mask32(*sp['S = -N'], 'iam1')).all()
    assert np.isnan(mc.ref_mask32(*sp['xi overflows'], 'irm2')).all() and np.isfinite(mc.ref_mask32(*sp['xi overflows'], 'irm1')).all()
    assert (np.abs(sp['|N| < EPS'][1]) < mc.EPS).all()


def test_ties_are_exact_and_the_reference_answers_one():
    for what, (S, N) in mc.tie_inputs().items():
        assert np.array_equal(np.abs(S), np.abs(N)), what
        for kind in ('ibm1', 'ibm2'):
            assert mc.ref_mask32(S, N, kind).all(), (what, kind)


def test_vad_restatement_of_the_kernel_agrees_with_the_oracle_on_1500_signals():
    rng = np.random.default_rng(3)
    n = 0
    while n < 1500:
        n_fft = (512, 1024)[n % 2]
        L = int(rng.choice(mc.vad_lengths(n_fft) + (int(rng.integers(n_fft // 2 + 1, 9000)),)))
        x = mc.vad_signals(L, rng)
        ref = mc.vad_reference(x, n_fft)[:, :, 0]
        for i, xi in enumerate(x):
            got = mc.vad_restatement(xi, n_fft)
            assert np.array_equal(got, ref[i, :len(got)]) and not ref[i, len(got):].any(), (n_fft, L, mc.VAD_FAMILIES[i])
        n += len(x)


def test_vad_lengths_hold_the_promised_edges():
    for n_fft in (512, 1024):
        hop = n_fft // 2
        Ls = mc.vad_lengths(n_fft)
        assert {n_fft, n_fft + 1, 3 * n_fft - 1, 3 * n_fft, 2501, 12801, 5000, 7001} <= set(Ls)
        assert any(hop < L < n_fft for L in Ls) and any(L % hop == 1 for L in Ls) and any(L % hop == hop - 1 for L in Ls)
    for L in (2501, 12801):
        assert (L - 1) * 99 % 100 == 0                                       # (L - 1) 0.99 is an integer
    x = mc.vad_signals(5000, np.random.default_rng(4))
    assert not x[5].any() and np.array_equal(x[4] * 8, np.round(x[4] * 8)) and (x[3] == 0).mean() > 0.4
    # heavy ties: the quantised family has far fewer distinct values than samples
    assert np.unique(x[4]).size < 100 and np.unique(x[2]).size < x[2].size


def test_band_banks_reach_every_signals_per_workgroup_edge():
    spb = {str(bank): mc.spb_of(mc.band_bank(bank)[0].shape[0]) for bank in mc.BANKS}
    assert [spb[str(k)] for k in (1, 7, 8, 9, 100, 129, 256)] == [32, 32, 32, 28, 2, 1, 1]
    assert 256 // 7 > 32 and any(256 % mc.band_bank(bank)[0].shape[0] for bank in mc.BANKS)
    assert {mc.band_bank('third16k')[0].shape[0], mc.band_bank('third8k')[0].shape[0]} <= set(range(10, 19))
    assert any(stop - start < 256 for _, start, stop in mc.SPANS) and any(stop == start for _, start, stop in mc.SPANS)


def test_scipy_distance_from_the_long_double_recurrence():
    """The 'ba' form is ill-conditioned in the low bands: SciPy's float64 lfilter is far from the long-double run there and at rounding
    level at the top, which is why the bar is per band."""
    r = mc.band_case('third16k', (700, 0, 700))['ungated']
    print('scipy distance per band (sum y^2):', np.array2string(r['scipy2'], precision=2))
    assert r['scipy2'][0] > 1e-7 and r['scipy2'][-1] < 1e-12
    # lfilter_ld restates lfilter: at the top band, where both are well conditioned, they agree to rounding
    ref = mc.band_case('third16k', (700, 3, 515))
    assert np.all(ref['ungated']['cnt'] == 515 - 140) and np.all(ref['gated']['cnt'] < 512)


def test_pair_shapes_and_mask_names():
    assert len(mc.NAMES) == 30 and mc.mask_bar(0) == 4 * mc.U and mc.mask_bar(1) == 14 * mc.U
    assert (2, 1000, 500, 500) in mc.PAIR_SHAPES and (3, 1, 0, 1) in mc.PAIR_SHAPES
    assert len(mc.channel_cases()) == 21
    assert mo.EPS == mc.EPS


def test_pooling_of_scipys_distance_over_neighbouring_bands():
    for bank in ('third16k', 'third8k'):
        fc = mc.band_bank(bank)[2]
        d = np.arange(1.0, fc.size + 1)
        assert np.array_equal(mc._pooled(d, fc), d)                      # a third of an octave apart: every band keeps its own figure
    fc = mc.band_bank(256)[2]
    d = np.random.default_rng(5).random(256)
    pooled = mc._pooled(d, fc)
    width = int(np.floor(255 / (6 * np.log2(6000 / 150))))              # bands within a sixth of an octave on either side
    assert width == 7 and np.all(pooled >= d) and pooled[100] == d[100 - width:100 + width + 1].max()
