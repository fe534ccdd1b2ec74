"""The float64 ESTOI yardstick of tests/estoi_checks.py on its own (no library, no GPU): against its whole-array form, against pystoi's
jittered form, closed forms, monotony in SNR, the preconditions of the compared cases and the float32 floor behind TOL_ESTOI."""
import numpy as np

import estoi_checks as ec


def test_yardstick_against_its_vectorised_form():
    worst = 0.0
    for fs, n in ec.CASES:
        for snr in ec.SNRS:
            a, b = ec.yard_of(1, n, fs, snr), ec.yard_of(1, n, fs, snr, vectorised=True)
            assert (a.status, a.n_kept, a.T, a.kept) == (b.status, b.n_kept, b.T, b.kept) and a.margin == b.margin
            worst = max(worst, abs(a.d - b.d))
    print(f'loops against whole arrays: worst |diff| = {worst:.3g}')
    assert worst < 1e-13


def test_jitter_of_pystoi_moves_nothing():
    """pystoi's form of the last stage (EPS randn before each normalisation, no EPS in the denominators) on the 54 compared cases."""
    worst = 0.0
    for i, (fs, n, seed, snr) in enumerate(ec.compared_cases()):
        x, y = ec.make_pair(seed, n, fs, snr)
        a, b = ec.yard_of(seed, n, fs, snr), ec.estoi_jittered(x, y, fs, 5000 + i)
        assert b.status == 0 and a.kept == b.kept
        worst = max(worst, abs(a.d - b.d))
    print(f'jittered (pystoi) form against the yardstick over {i + 1} cases: worst |diff| = {worst:.3g}')
    assert worst < 1e-12


def test_last_stage_loops_against_whole_arrays_on_exact_inputs():
    X, Y = ec.band_inputs(2, 29 + 64 + 5)
    for i in range(2):
        assert abs(ec._segments_loop(X[i], Y[i]) - ec._segments_vec(X[i], Y[i])) < 1e-13
    assert abs(ec._segments_loop(X[0], X[0]) - 1) < 1e-13 and ec._segments_loop(X[0], np.zeros_like(X[0])) == 0.0


def test_closed_forms():
    x, _ = ec.make_pair(1, 16000, 16000, 5.0)
    x = x.astype(np.float64)
    for scale in (1.0, 3.0, -1.0):                                    # the envelopes are magnitudes and every row is normalised
        d = ec.estoi_yardstick(x, scale * x, 16000).d
        print(f'y = {scale:+.0f} x: d {d:.15f}')
        assert abs(d - 1) < 1e-12


def test_d_falls_with_snr():
    for seed in ec.SEEDS:
        d = [ec.yard_of(seed, 16000, 16000, snr).d for snr in ec.SNRS]
        assert d[0] > d[1] > d[2], d


def test_compared_cases_meet_the_precondition():
    for fs, n, seed, snr in ec.compared_cases():
        ec.assert_precondition(ec.yard_of(seed, n, fs, snr), (fs, n, seed, snr))


def test_float32_floor():
    """Worst |float32-staged - float64| over the committed case list: the number behind TOL_ESTOI."""
    worst, margins, ds = 0.0, [], []
    for fs, n, seed, snr in ec.compared_cases():
        x, y = ec.make_pair(seed, n, fs, snr)
        a, b = ec.yard_of(seed, n, fs, snr), ec.estoi_f32_staged(x, y, fs)
        assert a.kept == b.kept
        worst = max(worst, abs(a.d - b.d))
        margins.append(a.margin)
        ds.append(a.d)
    def rule(floor):
        """16 x the floor, rounded up to one digit, capped at 5e-6"""
        digit = 10 ** np.floor(np.log10(16 * floor))
        return min(np.ceil(16 * floor / digit) * digit, 5e-6)

    print(f'float32 floor over {len(ds)} cases: {worst:.3g}; 16 x = {16 * worst:.3g} -> {rule(worst):.0e}; margins {min(margins):.3g} .. {max(margins):.3g} dB; '
          f'd {min(ds):.3f} .. {max(ds):.3f}')
    assert worst <= ec.FLOOR_MEASURED <= 2 * worst, (worst, ec.FLOOR_MEASURED)          # the committed figure is the measured one
    assert np.isclose(ec.TOL_ESTOI, rule(ec.FLOOR_MEASURED), rtol=1e-9), (ec.TOL_ESTOI, rule(ec.FLOOR_MEASURED))


def test_segments_constant_is_stated_once():
    assert ec.segs_per_workgroup() == 64
