"""Checks of the ESTOI kernels (csrc/k_estoi.h: disco_estoi, disco_estoi_bands) and their Python surface (Engine.estoi, Engine.estoi_bands,
disco_amd.metrics.estoi, results_io.room_results / batch_results(estoi=True)), shared by tests/test_estoi_cpu.py (no library),
tests/test_estoi_emulated.py (hipemu) and tests/test_gpu_estoi.py (MI355X).

ESTOI (Jensen & Taal 2016) is what pystoi computes with extended=True.  pystoi is third-party and absent, so the measure is restated here
from its definition as a float64 YARDSTICK (`estoi_yardstick`: plain loops over frames, segments, rows and columns); the inputs and the
front half (resampling, kept frames, band table, window) are those of tests/stoi_checks.py, imported.  `estoi_vectorised` is the same
arithmetic on whole arrays, `estoi_f32_staged` the same with the stages the kernels run in float32 run in float32 (the staging of
stoi_checks._staged).  pystoi adds EPS randn to every segment before each of its two normalisations so that it never divides by zero;
neither the kernels nor the yardstick reproduce that jitter (`estoi_jittered` does, with a seeded generator: it moves d by some 1e-15 on
the compared cases, test_estoi_cpu.py holds it under 1e-12).  Without it the result is deterministic and a row or column whose centred norm
is exactly 0 contributes 0 through the "+ EPS" of its denominator.  Nothing here is pinned against the package.

Tolerance.  TOL_ESTOI bounds |d_kernel - d_yardstick|, by the rule of stoi_checks.TOL_STOI: set from the float32 floor -- the worst
|estoi_f32_staged - estoi_yardstick| over CASES x SEEDS x SNRS, which test_estoi_cpu.py::test_float32_floor measures and prints -- never
from a kernel's output: 16 x the floor (the factor is for the kernel's radix-8 Stockham FFT with float32 twiddles and a summation order
other than pocketfft's), rounded up to one digit, capped at 5e-6.
Measured floor: 6.7e-8 (54 cases; margins 0.40 .. 9.4 dB, d 0.158 .. 0.887)  ->  16 x = 1.1e-6  ->  TOL_ESTOI = 2e-6."""
import functools
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import scipy.fft

import stoi_checks as sc
from stoi_checks import CASES, EPS, FS, HOP, N_FRAME, N_SEG, NFFT, NUMBAND, SEEDS, SNRS, Yard, band_table, make_pair, resample, window

FLOOR_MEASURED = 6.7e-8
TOL_ESTOI = 2e-6
assert TOL_ESTOI <= 5e-6

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ----------------------------------------------------------------------------------------------------------
def _segments_loop(X, Y):
    """The last stage in float64, by loops: X, Y (15, T) -> d."""
    T = X.shape[1]
    J = T - N_SEG + 1
    total = 0.0
    for m in range(J):
        Xn, Yn = np.zeros((NUMBAND, N_SEG)), np.zeros((NUMBAND, N_SEG))
        for A, An in ((X, Xn), (Y, Yn)):
            for b in range(NUMBAND):                                                     # rows: over the 30 frames
                row = A[b, m:m + N_SEG].astype(np.float64)
                row = row - np.sum(row) / N_SEG
                An[b] = row / (np.sqrt(np.sum(row * row)) + EPS)
            for n in range(N_SEG):                                                       # columns: over the 15 bands
                col = An[:, n] - np.sum(An[:, n]) / NUMBAND
                An[:, n] = col / (np.sqrt(np.sum(col * col)) + EPS)
        total += float(np.sum(Xn * Yn)) / N_SEG
    return total / J


def _segments_vec(X, Y, rng=None):
    """The same on whole arrays.  rng: pystoi's form instead -- EPS randn added before each normalisation, no EPS in the denominators."""
    T = X.shape[1]
    idx = np.arange(N_SEG)[None, :] + np.arange(T - N_SEG + 1)[:, None]
    out = []
    for A in (X, Y):
        a = np.transpose(A[:, idx].astype(np.float64), (1, 0, 2))                        # (J, 15, 30)
        for axis in (2, 1):
            if rng is not None:
                a = a + EPS * rng.standard_normal(a.shape)
            a = a - np.mean(a, axis=axis, keepdims=True)
            a = a / (np.sqrt(np.sum(a * a, axis=axis, keepdims=True)) + (EPS if rng is None else 0.0))
        out.append(a)
    return float(np.sum(out[0] * out[1]) / N_SEG / idx.shape[0])


def envelopes_loop(x, y, fs_sig):
    """The front half of stoi_checks.stoi_yardstick: -> (X, Y (15, T) float64 or None without a frame, kept, margin)."""
    x10, y10 = resample(x, fs_sig), resample(y, fs_sig)
    w = window()
    starts, kept, margin = sc._keep(x10)
    if not starts:
        return None, None, kept, margin
    nk = len(kept)
    xs, ys = np.zeros((nk - 1) * HOP + N_FRAME), np.zeros((nk - 1) * HOP + N_FRAME)
    for k, f in enumerate(kept):
        i = starts[f]
        xs[k * HOP:k * HOP + N_FRAME] += w * x10[i:i + N_FRAME]
        ys[k * HOP:k * HOP + N_FRAME] += w * y10[i:i + N_FRAME]
    lo, hi = band_table()
    fr = list(range(0, len(xs) - N_FRAME, HOP))
    X, Y = np.zeros((NUMBAND, len(fr))), np.zeros((NUMBAND, len(fr)))
    for t, i in enumerate(fr):
        sx, sy = np.fft.rfft(w * xs[i:i + N_FRAME], NFFT), np.fft.rfft(w * ys[i:i + N_FRAME], NFFT)
        for b in range(NUMBAND):
            X[b, t] = np.sqrt(np.sum(np.abs(sx[lo[b]:hi[b]]) ** 2))
            Y[b, t] = np.sqrt(np.sum(np.abs(sy[lo[b]:hi[b]]) ** 2))
    return X, Y, kept, margin


def envelopes_staged(x, y, fs_sig, dt):
    """Whole-array form of the front half (stoi_checks._staged); dt = float64: the yardstick's arithmetic; float32: the kernels' staging."""
    x10, y10 = resample(x, fs_sig).astype(dt), resample(y, fs_sig).astype(dt)
    w = window().astype(dt)
    starts, kept, margin = sc._keep(x10)
    if not starts:
        return None, None, kept, margin
    nk = len(kept)
    sel = np.array(starts)[kept][:, None] + np.arange(N_FRAME)[None, :]
    T = nk - 1
    lo, hi = band_table()
    tob = []
    for s in (x10, y10):
        fr = w * s[sel]                                                                  # (nk, 256)
        o = np.zeros((nk + 1, HOP), dt)
        o[:-1] += fr[:, :HOP]
        o[1:] += fr[:, HOP:]
        o = o.reshape(-1)
        fr = w * o[(np.arange(T) * HOP)[:, None] + np.arange(N_FRAME)[None, :]] if T > 0 else np.zeros((0, N_FRAME), dt)
        sp = scipy.fft.rfft(fr, NFFT, axis=-1)
        assert sp.dtype == (np.complex64 if dt == np.float32 else np.complex128)
        pw = sp.real * sp.real + sp.imag * sp.imag
        tob.append(np.sqrt(np.stack([np.sum(pw[:, lo[b]:hi[b]], axis=-1, dtype=dt) for b in range(NUMBAND)])))
    return tob[0], tob[1], kept, margin


def _score(env, last_stage):
    X, Y, kept, margin = env
    if X is None:
        return Yard(np.nan, 2, 0, -1, margin, kept)
    T = X.shape[1]
    if T < N_SEG:
        return Yard(1e-5, 1, len(kept), T, margin, kept)
    return Yard(last_stage(X, Y), 0, len(kept), T, margin, kept)


def estoi_yardstick(x, y, fs_sig):
    """The float64 yardstick, straight from the definition."""
    return _score(envelopes_loop(x, y, fs_sig), _segments_loop)


def estoi_vectorised(x, y, fs_sig):
    return _score(envelopes_staged(x, y, fs_sig, np.float64), _segments_vec)


def estoi_f32_staged(x, y, fs_sig):
    return _score(envelopes_staged(x, y, fs_sig, np.float32), _segments_vec)


def estoi_jittered(x, y, fs_sig, seed):
    """pystoi's own form of the last stage (random jitter, no EPS in the denominators) on the yardstick's envelopes."""
    rng = np.random.default_rng(seed)
    return _score(envelopes_staged(x, y, fs_sig, np.float64), lambda X, Y: _segments_vec(X, Y, rng))


@functools.lru_cache(maxsize=None)
def yard_of(seed, n, fs_sig, kind, vectorised=False):
    x, y = make_pair(seed, n, fs_sig, kind)
    return (estoi_vectorised if vectorised else estoi_yardstick)(x, y, fs_sig)


def compared_cases():
    return sc.compared_cases()


def assert_precondition(yd, what):
    """Asserted, not skipped: the keep decision is not on a knife's edge and d is in the range where ESTOI discriminates."""
    assert yd.status == 0, (what, yd.status)
    assert yd.margin >= 0.01, (what, 'keep-threshold margin', yd.margin)
    assert 0.1 < yd.d < 0.95, (what, 'd', yd.d)


def segs_per_workgroup():
    """S, the segments one workgroup of k_estoi_corr owns: mirrored in disco_amd._lib, asserted against the header and the kernel source."""
    from disco_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'disco_hip.h')).read()
    src = open(os.path.join(REPO, 'disco_amd', 'csrc', 'k_estoi.h')).read()
    in_hdr = int(re.search(r'#define\s+DISCO_ESTOI_SEGS\s+(\d+)', hdr).group(1))
    in_src = int(re.search(r'constexpr\s+int\s+ESTOI_SEGS\s*=\s*(\d+)\s*;', src).group(1))
    assert _lib.ESTOI_SEGS == in_hdr == in_src, (_lib.ESTOI_SEGS, in_hdr, in_src)
    return in_src


# ---- checks through the library ------------------------------------------------------------------------------------------------
def _eng():
    from disco_amd import metrics as dm
    return dm._engine()


def check_against_yardstick(fs_sig, n):
    """All seeds and SNRs of one (fs, n) in one batch, through Engine.estoi and metrics.estoi."""
    from disco_amd import metrics as dm
    keys = [(seed, snr) for seed in SEEDS for snr in SNRS]
    x = np.stack([make_pair(seed, n, fs_sig, snr)[0] for seed, snr in keys])
    y = np.stack([make_pair(seed, n, fs_sig, snr)[1] for seed, snr in keys])
    d, status, kept = _eng().estoi(x, y, fs_sig, want_kept=True)
    d2 = dm.estoi(x.reshape(3, 3, n), y.reshape(3, 3, n), fs_sig)
    assert d2.shape == (3, 3) and np.array_equal(d2.reshape(-1), d)
    worst = 0.0
    for i, (seed, snr) in enumerate(keys):
        yd = yard_of(seed, n, fs_sig, snr)
        assert_precondition(yd, (fs_sig, n, seed, snr))
        err = abs(d[i] - yd.d)
        worst = max(worst, err)
        print(f'fs {fs_sig} n {n} seed {seed} snr {snr:+.0f}: d {d[i]:.9f} yardstick {yd.d:.9f} |err| {err:.3g} kept {kept[i]}/{len(yd.kept)} margin {yd.margin:.3g} dB')
        assert status[i] == 0 and kept[i] == yd.n_kept
        assert err < TOL_ESTOI, (fs_sig, n, seed, snr, d[i], yd.d)
    print(f'fs {fs_sig} n {n}: worst |err| = {worst:.3g} (TOL_ESTOI {TOL_ESTOI:g})')


def band_inputs(n_pair, tmax, seed=11):
    """Envelopes uniform in [0.5, 1.5], rounded to float32: well conditioned by construction."""
    rng = np.random.default_rng(4000 + seed)
    return (rng.uniform(0.5, 1.5, (n_pair, NUMBAND, tmax)).astype(np.float32), rng.uniform(0.5, 1.5, (n_pair, NUMBAND, tmax)).astype(np.float32))


def assert_well_conditioned(A):
    """Every centred row (band, segment) of A (15, T) keeps more than 1e-2 of the row's norm."""
    T = A.shape[1]
    idx = np.arange(N_SEG)[None, :] + np.arange(T - N_SEG + 1)[:, None]
    a = A[:, idx].astype(np.float64)
    c = a - np.mean(a, axis=-1, keepdims=True)
    ratio = np.sqrt(np.sum(c * c, axis=-1)) / np.sqrt(np.sum(a * a, axis=-1))
    assert np.min(ratio) > 1e-2, np.min(ratio)


def check_bands_frame_counts():
    """Engine.estoi_bands on exact inputs: every T around the workgroup's run of S segments in one batch through `frames` (workgroups past
    a pair's J return early), each pair bit for bit what it gives alone, and within 1e-12 of the yardstick's last stage -- fewer than 1e3
    float64 operations on values of magnitude <= 1 per segment, averaged."""
    S = segs_per_workgroup()
    eng = _eng()
    Ts = [29, 30, 31, 29 + S - 1, 29 + S, 29 + S + 1, 29 + 2 * S + 3]
    tmax = max(Ts)
    X, Y = band_inputs(len(Ts), tmax)
    d, status = eng.estoi_bands(X, Y, frames=np.array(Ts))
    worst = 0.0
    for i, T in enumerate(Ts):
        alone, st_alone = eng.estoi_bands(X[i:i + 1], Y[i:i + 1], frames=np.array([T]))
        cut, st_cut = eng.estoi_bands(np.ascontiguousarray(X[i:i + 1, :, :T]), np.ascontiguousarray(Y[i:i + 1, :, :T]))       # frames = None: tmax
        assert alone[0] == d[i] == cut[0] and st_alone[0] == status[i] == st_cut[0], (T, d[i], alone, cut)
        if T < N_SEG:
            assert status[i] == 1 and d[i] == 1e-5, (T, d[i], status[i])
            continue
        assert_well_conditioned(X[i, :, :T])
        assert_well_conditioned(Y[i, :, :T])
        want = _segments_loop(X[i, :, :T], Y[i, :, :T])
        worst = max(worst, abs(d[i] - want))
        print(f'estoi_bands T {T} (J {T - 29}): d {d[i]:+.15f} yardstick {want:+.15f} |err| {abs(d[i] - want):.3g}')
        assert status[i] == 0 and abs(d[i] - want) < 1e-12, (T, d[i], want)
    print(f'estoi_bands: worst |err| = {worst:.3g} over T = {Ts}')
    with pytest.raises(ValueError):
        eng.estoi_bands(X, Y, frames=np.array(Ts) + 1)                                  # one frame count beyond tmax
    with pytest.raises(ValueError):
        eng.estoi_bands(X, Y[:, :, :-1])


def check_bands_degenerate():
    """Degeneracies that are exact in any summation order.  Columns that vanish only up to rounding (all bands equal, say) are NOT tested:
    their centred norm is some 1e-16 next to EPS, so their value is undetermined here, as it is random in pystoi."""
    S = segs_per_workgroup()
    eng = _eng()
    T = 29 + S + 11
    X, Y = band_inputs(3, T, seed=12)
    # a band whose 30 values all equal 1.0 within the segments 40 .. 50: its centred row is exactly 0 and contributes exactly 0
    Xc = X.copy()
    Xc[0, 3, 40:80] = 1.0
    d, status = eng.estoi_bands(Xc, Y)
    want = _segments_loop(Xc[0], Y[0])
    idx = np.arange(N_SEG)[None, :] + np.arange(T - N_SEG + 1)[:, None]
    flat = np.flatnonzero(np.all(Xc[0, 3][idx] == 1.0, axis=1))
    assert flat.tolist() == list(range(40, 51))
    print(f'constant band: d {d[0]:+.15f} yardstick {want:+.15f}')
    assert np.all(status == 0) and np.isfinite(d[0]) and abs(d[0] - want) < 1e-12, (d[0], want)
    base, _ = eng.estoi_bands(X, Y)
    assert np.array_equal(d[1:], base[1:]) and d[0] != base[0]
    # Y = 0: every product is an exact 0
    d0, st0 = eng.estoi_bands(X, np.zeros_like(Y))
    assert np.all(st0 == 0) and np.all(d0 == 0.0), d0
    assert _segments_loop(X[0], np.zeros_like(Y[0])) == 0.0
    # X = Y: every column correlates with itself
    d1, st1 = eng.estoi_bands(X, X.copy())
    assert np.all(st1 == 0) and np.all(np.abs(d1 - 1) < 1e-12), d1
    # a NaN in one envelope sample of pair 0: its d is NaN, the other pairs keep their bits
    Xn = X.copy()
    Xn[0, 7, 33] = np.nan
    dn, stn = eng.estoi_bands(Xn, Y)
    assert np.isnan(dn[0]) and np.array_equal(dn[1:], base[1:]) and np.all(stn == 0), dn


def check_frame_count_edges():
    """stoi_checks.edge_cases() and the spans without a frame through the whole call."""
    from disco_amd import metrics as dm
    cases = sc.edge_cases()
    for name in ('T29', 'T30', 'T31'):
        x, y, want_kept = cases[name]
        yd = estoi_yardstick(x, y, FS)
        NF = len(range(0, len(x) - N_FRAME, HOP))
        assert yd.kept == want_kept(NF) and yd.margin >= 0.01 and yd.T == int(name[1:]), (name, yd.kept, yd.margin, yd.T)
        d, status, kept = _eng().estoi(x[None], y[None], FS, want_kept=True)
        print(f'{name}: n10 {len(x)} frames {NF} kept {kept[0]} T {yd.T} d {d[0]:.9f} yardstick {yd.d:.9f} status {status[0]}')
        assert kept[0] == yd.n_kept and status[0] == yd.status
        if name == 'T29':
            assert status[0] == 1 and d[0] == 1e-5
            with pytest.warns(RuntimeWarning):
                assert dm.estoi(x, y, FS) == 1e-5
        else:
            assert status[0] == 0 and abs(d[0] - yd.d) < TOL_ESTOI, (name, d[0], yd.d)
            with warnings.catch_warnings():
                warnings.simplefilter('error')
                assert dm.estoi(x, y, FS) == d[0]
    x, y = sc.edge_signal(2000)
    for fs_sig, n in ((FS, 256), (16000, 409), (FS, 1)):                                   # ceil(409 * 5 / 8) = 256: no frame at all
        d, status = _eng().estoi(x[None, :n], y[None, :n], fs_sig)
        assert status[0] == 2 and np.isnan(d[0]), (fs_sig, n, d, status)
        with pytest.raises(ValueError, match='pair'):
            dm.estoi(x[:n], y[:n], fs_sig)
    with pytest.raises(ValueError, match=r'pair \(1, 0\)'):
        dm.estoi(np.stack([x, x])[:, None], np.stack([y, y])[:, None], FS, stop=np.array([[2000], [100]]))
    with pytest.raises(ValueError):
        dm.estoi(x, y[:-1], FS)


def check_all_zero_x_and_identity():
    from disco_amd import metrics as dm
    xs, y = make_pair(1, 16000, 16000, 5.0)
    for fs_sig in (16000, FS):
        d, status, kept = _eng().estoi(np.zeros((1, 16000), np.float32), y[None], fs_sig, want_kept=True)
        assert status[0] == 0 and d[0] == 0.0 and not np.isnan(d[0]), (d, status)
        assert kept[0] == len(range(0, (16000 * FS // fs_sig) - N_FRAME, HOP))            # equal energies: every frame kept
    assert dm.estoi(np.zeros(16000, np.float32), y, 16000) == 0.0
    assert estoi_yardstick(np.zeros(16000, np.float32), y, 16000).d == 0.0
    yd = estoi_yardstick(xs, xs, 16000)                                                    # y == x
    d, status = _eng().estoi(xs[None], xs[None], 16000)
    print(f'y == x: d {d[0]:.12f} yardstick {yd.d:.12f}')
    assert status[0] == 0 and abs(yd.d - 1) < 1e-9 and abs(d[0] - yd.d) < TOL_ESTOI, (d[0], yd.d)


def check_bit_identity(n=16003, fs_sig=16000):
    """Alone, in a batch of 24, in a batch walked under a tiny budget; per-pair stop against slices; start / stop against slicing; and
    Engine.stoi before and after an Engine.estoi call on the same engine: the shared stages leave STOI alone."""
    eng = _eng()
    kinds = (20.0, 5.0, -5.0, 'filt')
    x = np.stack([make_pair(1 + i % 3, n, fs_sig, kinds[i % 4])[0] for i in range(24)])
    y = np.stack([make_pair(1 + i % 3, n, fs_sig, kinds[i % 4])[1] for i in range(24)])
    stoi_before = eng.stoi(x, y, fs_sig)
    d, status = eng.estoi(x, y, fs_sig)
    stoi_after = eng.stoi(x, y, fs_sig)
    assert np.array_equal(stoi_before[0], stoi_after[0]) and np.array_equal(stoi_before[1], stoi_after[1])
    assert not np.any(d == stoi_before[0])
    assert np.all(status == 0) and len(set(d.tolist())) == 12
    assert np.array_equal(d[:6], eng.estoi(x[:6], y[:6], fs_sig)[0])                       # run to run, and a smaller batch
    for i in (7, 23):
        assert eng.estoi(x[i:i + 1], y[i:i + 1], fs_sig)[0][0] == d[i], i
    per_pair = eng.lib.disco_estoi_workspace_bytes(eng.ctx, 1, n, 5, 8, 581)
    d5, st5 = eng.estoi(x, y, fs_sig, budget_bytes=5 * per_pair + 4096)                    # chunks of 5, 5, 5, 5, 4
    assert np.array_equal(d5, d) and np.array_equal(st5, status)
    d1, st1 = eng.estoi(x[:3], y[:3], fs_sig, budget_bytes=1)                              # one pair per call
    assert np.array_equal(d1, d[:3]) and np.array_equal(st1, status[:3])
    # per-pair stop: every pair as if sliced and scored alone
    start = 37
    stops = np.array([n - 13 * i for i in range(24)])
    stops[5] = start + 300                                                                 # too short for a frame
    stops[6] = start + 3000                                                                # a dozen frames: 1e-5
    dp, sp = eng.estoi(x, y, fs_sig, start=start, stop=stops)
    for i in (0, 5, 6, 11, 23):
        da, sa = eng.estoi(np.ascontiguousarray(x[i:i + 1, start:stops[i]]), np.ascontiguousarray(y[i:i + 1, start:stops[i]]), fs_sig)
        assert sa[0] == sp[i] and (da[0] == dp[i] or (np.isnan(da[0]) and np.isnan(dp[i]))), (i, da, dp[i])
    assert sp[5] == 2 and sp[6] == 1 and dp[6] == 1e-5 and np.all(np.delete(sp, (5, 6)) == 0)
    # scalar start / stop equals slicing; at 10 kHz too (no resampled copy: the kernels read the caller's rows from `start`)
    for fs2 in (fs_sig, FS):
        ds, ss = eng.estoi(x[:4], y[:4], fs2, start=101, stop=n - 55)
        dsl, ssl = eng.estoi(np.ascontiguousarray(x[:4, 101:n - 55]), np.ascontiguousarray(y[:4, 101:n - 55]), fs2)
        assert np.array_equal(ds, dsl) and np.array_equal(ss, ssl) and np.all(ss == 0)
    with pytest.raises(ValueError):
        eng.estoi(x, y, fs_sig, start=5, stop=n + 1)
    with pytest.raises(ValueError):
        eng.estoi(x, y[:, :-1], fs_sig)


def check_device_resident(n=9603, fs_sig=16000):
    """Device-resident inputs are read in place, chunked or not: the same bits as the NumPy route; estoi_bands likewise."""
    import torch
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    x = np.stack([make_pair(1 + i % 3, n, fs_sig, 5.0)[0] for i in range(6)])
    y = np.stack([make_pair(1 + i % 3, n, fs_sig, 5.0)[1] for i in range(6)])
    eng = _eng()
    d, _ = eng.estoi(x, y, fs_sig)
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    assert np.array_equal(eng.estoi(tx, ty, fs_sig)[0], d)
    assert np.array_equal(eng.estoi(tx, ty, fs_sig, budget_bytes=1)[0], d)
    X, Y = band_inputs(2, 70, seed=13)
    assert np.array_equal(eng.estoi_bands(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev))[0], eng.estoi_bands(X, Y)[0])


def check_room_results(tmp_path, fs=16000):
    """room_results(stoi=True, estoi=True): the four new keys equal differences of metrics.estoi values computed directly; estoi=False
    gives exactly the key sets of before; the pickle writers carry the extra keys through."""
    from disco_amd import metrics as dm
    from disco_amd.speech_enhancement import results_io as rio
    g = sc.stoi_room()
    K = g['s_in'].shape[0]
    kw = dict(rnd_snrs=[3.0], fs=fs)
    pos = [g[k] for k in ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')]
    times = dict(y_in=g['y_in'], sh_t=g['sh_t'], szh_t=g['szh_t'])
    assert rio.ESTOI_KEYS_TANGO == ('delta_estoi_cnv', 'delta_estoi_dry') and rio.ESTOI_KEYS_MWF == ('delta_estoi', 'delta_estoi_dry')
    res, resz = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], bss_flen=8, stoi=True, estoi=True, **times, **kw)
    assert tuple(res) == rio.RESULT_KEYS_TANGO + rio.ESTOI_KEYS_TANGO and tuple(resz) == rio.RESULT_KEYS_MWF + rio.ESTOI_KEYS_MWF
    cut = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)[..., fs:])
    for k in range(K):
        for clean, key_t, key_z in ((g['s_in'][k], 'delta_estoi_cnv', 'delta_estoi'), (g['s_dry'], 'delta_estoi_dry', 'delta_estoi_dry')):
            d_in, d_out, d_z = (dm.estoi(cut(clean), cut(e), fs) for e in (g['y_in'][k], g['sh_t'][k], g['szh_t'][k]))
            print(f'node {k} {key_t}: {res[key_t][k]:.9f}  {key_z} (resz): {resz[key_z][k]:.9f}')
            assert res[key_t][k] == d_out - d_in and resz[key_z][k] == d_z - d_in, (k, key_t)
            yd_in, yd_out = (estoi_vectorised(cut(clean), cut(e), fs) for e in (g['y_in'][k], g['sh_t'][k]))
            assert yd_in.status == 0 and yd_out.status == 0 and min(yd_in.margin, yd_out.margin) >= 0.01
            assert abs(res[key_t][k] - (yd_out.d - yd_in.d)) < 2 * TOL_ESTOI, (key_t, k, res[key_t][k], yd_out.d - yd_in.d)
    assert not np.array_equal(res['delta_estoi_cnv'], res['delta_stoi_cnv']) and not np.array_equal(res['delta_estoi_dry'], resz['delta_estoi_dry'])
    # estoi=False, the default: exactly the key sets and the values of before
    r0, rz0 = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], bss_flen=8, stoi=True, **times, **kw)
    assert tuple(r0) == rio.RESULT_KEYS_TANGO and tuple(rz0) == rio.RESULT_KEYS_MWF
    for r, rr in ((res, r0), (resz, rz0)):
        for key in rr:
            assert np.array_equal(np.asarray(r[key]), np.asarray(rr[key]), equal_nan=True), key
    # without the dry sources the _dry keys stay NaN; without the time signals every ESTOI key is NaN
    r1, rz1 = rio.room_results(*pos, bss_flen=8, estoi=True, **times, **kw)
    assert np.array_equal(r1['delta_estoi_cnv'], res['delta_estoi_cnv']) and np.array_equal(rz1['delta_estoi'], resz['delta_estoi'])
    assert np.all(np.isnan(r1['delta_estoi_dry'])) and np.all(np.isnan(rz1['delta_estoi_dry'])) and np.all(np.isnan(r1['delta_stoi_cnv']))
    r2, rz2 = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], estoi=True, **kw)
    assert all(np.all(np.isnan(r[key])) for r, keys in ((r2, rio.ESTOI_KEYS_TANGO), (rz2, rio.ESTOI_KEYS_MWF)) for key in keys)
    files = rio.write_result_pickles(str(tmp_path), 11001, 'ssn', res, resz)
    for f, r in zip(files, (res, resz)):
        back = pickle.load(open(f, 'rb'))
        assert set(back) == set(r)
        for key in rio.ESTOI_KEYS_TANGO + rio.ESTOI_KEYS_MWF:
            assert key not in r or np.array_equal(back[key], r[key])


def check_batch_results(fs=16000):
    """batch_results(estoi=True) on two rooms of different lengths: each room's row is that room scored alone at its own length."""
    from disco_amd.speech_enhancement import results_io as rio
    rooms = [sc.stoi_room(seed=5), sc.stoi_room(seed=6)]
    L = rooms[0]['s_in'].shape[-1]
    lens = np.array([L, L - 2001])
    names = ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')
    stack = lambda nm: np.stack([g[nm] for g in rooms])
    kw = dict(rnd_snrs=np.array([[3.0], [1.0]]), fs=fs, bss_flen=8)
    res, resz = rio.batch_results(*(stack(nm) for nm in names), s_dry=stack('s_dry'), n_dry=stack('n_dry'), y_in=stack('y_in'), sh_t=stack('sh_t'),
                                  szh_t=stack('szh_t'), stoi=True, estoi=True, lengths=lens, **kw)
    assert tuple(res) == rio.RESULT_KEYS_TANGO + rio.ESTOI_KEYS_TANGO and tuple(resz) == rio.RESULT_KEYS_MWF + rio.ESTOI_KEYS_MWF
    for r, g in enumerate(rooms):
        c = lambda nm: g[nm][..., :lens[r]]
        one, onez = rio.room_results(*(c(nm) for nm in names), rnd_snrs=[3.0], fs=fs, bss_flen=8, s_dry=c('s_dry'), n_dry=c('n_dry'), y_in=c('y_in'),
                                     sh_t=c('sh_t'), szh_t=c('szh_t'), stoi=True, estoi=True)
        for got, want, keys in ((res, one, rio.ESTOI_KEYS_TANGO), (resz, onez, rio.ESTOI_KEYS_MWF)):
            for key in keys + ('delta_stoi_dry',):
                print(f'room {r} {key}: {got[key][r]}')
                assert np.all(np.isfinite(got[key][r])) and np.array_equal(got[key][r], want[key]), (r, key, got[key][r], want[key])
    b0, bz0 = rio.batch_results(*(stack(nm) for nm in names), s_dry=stack('s_dry'), n_dry=stack('n_dry'), y_in=stack('y_in'), sh_t=stack('sh_t'),
                                szh_t=stack('szh_t'), lengths=lens, **kw)
    assert tuple(b0) == rio.RESULT_KEYS_TANGO and tuple(bz0) == rio.RESULT_KEYS_MWF                # estoi=False: the key sets of before
    assert all(np.array_equal(np.asarray(b0[k]), np.asarray(res[k]), equal_nan=True) for k in b0 if k not in rio.STOI_KEYS)


def check_surface():
    """metrics.stoi(extended=True) still refuses, now pointing to estoi; the refusals of disco_estoi return the documented codes, name the
    entry point and leave `out` untouched."""
    from disco_amd import _lib
    from disco_amd import metrics as dm
    x, y = sc.edge_signal(12000)
    with pytest.raises(NotImplementedError, match='estoi'):
        dm.stoi(x, y, FS, extended=True)
    eng = _eng()
    n, L = 2, 12000
    p, q, taps = sc.resample_taps(16000)
    px, kx = eng.to_device(np.stack([x, x]), np.float32)
    py, ky = eng.to_device(np.stack([y, y]), np.float32)
    pt, kt = eng.to_device(taps, np.float64)
    need = eng.lib.disco_estoi_workspace_bytes(eng.ctx, n, L, p, q, len(taps))
    assert need > 0 and eng.lib.disco_estoi_workspace_bytes(eng.ctx, n, L, p, q, len(taps) + 1) == 0
    ws = eng.empty((need // 8 + 1,), np.float64)
    sentinel = np.full((n, 2), -7.25)
    po, out = eng.to_device(sentinel, np.float64)
    pst, st = eng.to_device(np.full((n,), -3, np.int32), np.int32)
    call = lambda start, n_taps, ws_bytes: eng.lib.disco_estoi(eng.ctx, px, py, n, L, start, None, p, q, pt, n_taps, po, pst, ws.ptr, ws_bytes, eng.stream)
    for args, code, msg in (((L + 1, len(taps), ws.nbytes), _lib.E_ARG, 'disco_estoi: need 0 <= start <= len'),
                            ((-1, len(taps), ws.nbytes), _lib.E_ARG, 'disco_estoi: need 0 <= start <= len'),
                            ((0, len(taps) - 1, ws.nbytes), _lib.E_ARG, 'disco_estoi: resampling needs an odd number of taps (2 L + 1)'),
                            ((0, len(taps), need - 8), _lib.E_ARG, 'disco_estoi: workspace smaller than disco_estoi_workspace_bytes'),
                            ((0, (1 << 16) + 1, ws.nbytes), _lib.E_UNSUPPORTED, 'disco_estoi: resampling filters of at most 65536 taps')):
        assert call(*args) == code, args
        assert eng.lib.disco_last_error(eng.ctx).decode() == msg
        eng.sync()
        assert np.array_equal(out.numpy(), sentinel) and np.all(st.numpy() == -3), args
    assert call(0, len(taps), ws.nbytes) == 0
    eng.sync()
    assert np.all(st.numpy() == 0) and np.all(out.numpy()[:, 0] != -7.25)


def check_real_span(n=144000, fs_sig=16000, n_pair=24):
    """The span the reference scores (9 s at 16 kHz) as room_results issues it for one room of 4 nodes: 24 pairs in one call."""
    keys = [(1 + i % 3, SNRS[(i // 3) % 3]) for i in range(n_pair)]
    x = np.stack([make_pair(seed, n, fs_sig, snr)[0] for seed, snr in keys])
    y = np.stack([make_pair(seed, n, fs_sig, snr)[1] for seed, snr in keys])
    d, status, kept = _eng().estoi(x, y, fs_sig, want_kept=True)
    worst = 0.0
    for i, (seed, snr) in enumerate(keys):
        yd = yard_of(seed, n, fs_sig, snr, vectorised=i >= 2)           # the loops on two pairs, their whole-array form (test_estoi_cpu.py) on the rest
        assert_precondition(yd, (seed, snr))
        worst = max(worst, abs(d[i] - yd.d))
        assert status[i] == 0 and kept[i] == yd.n_kept and abs(d[i] - yd.d) < TOL_ESTOI, (seed, snr, d[i], yd.d)
    print(f'{n_pair} pairs of {n} samples: worst |err| = {worst:.3g}; d', d[:9])
