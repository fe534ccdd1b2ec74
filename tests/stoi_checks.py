"""Checks of the STOI kernels (csrc/k_stoi.h: disco_stoi) and their Python surface (Engine.stoi, disco_amd.metrics.stoi,
results_io.room_results(stoi=True)), shared by tests/test_stoi_cpu.py (no library), tests/test_stoi_emulated.py (hipemu) and
tests/test_gpu_stoi.py (MI355X).

pystoi is third-party and absent, so the measure is restated here from its definition (Taal, Hendriks, Heusdens, Jensen 2011, with the
constants and conventions pystoi uses) as a float64 YARDSTICK: NumPy, scipy.signal.resample_poly, plain loops over frames and segments
(`stoi_yardstick`).  `stoi_vectorised` is the same arithmetic on whole arrays, `stoi_f32_staged` the same with the stages the kernels
run in float32 run in float32 (resampling in float64 then rounded, framing, windowing, scipy.fft.rfft and band sums in float32,
the segment correlation in float64).  Nothing here is pinned against the package.

Tolerance.  TOL_STOI bounds |d_kernel - d_yardstick|.  It is set from the float32 floor -- the worst |stoi_f32_staged - stoi_yardstick|
over CASES x SEEDS x SNRS, which test_stoi_cpu.py::test_float32_floor measures and prints -- never from a kernel's output:
16 x the floor, rounded up to one digit, capped at 1e-6.  The factor 16 is for the kernel's radix-8 Stockham FFT with float32
twiddles and a summation order other than pocketfft's.  Measured floor: 3.2e-8 (54 cases; margins 0.40 .. 9.4 dB, d 0.45 .. 0.99)  ->  16 x = 5.1e-7  ->  TOL_STOI = 6e-7."""
import functools
import math
import pickle
import warnings

import numpy as np
import pytest
import scipy.fft
import scipy.signal

FS, N_FRAME, NFFT, NUMBAND, MINFREQ, N_SEG, BETA, DYN_RANGE = 10000, 256, 512, 15, 150, 30, -15.0, 40.0
EPS = 2.220446049250313e-16
HOP = N_FRAME // 2

FLOOR_MEASURED = 3.2e-8
TOL_STOI = 6e-7
assert TOL_STOI <= 1e-6

# (fs_sig, samples): 16 kHz spans with every n mod 8 class that changes ceil(5 n / 8), one each at 8 kHz and 10 kHz
CASES = ((16000, 16000), (16000, 16003), (16000, 20000), (16000, 24001), (8000, 9001), (10000, 11000))
SEEDS = (1, 2, 3)
SNRS = (20.0, 5.0, -5.0)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def resample_taps(fs_sig):
    g = math.gcd(FS, int(fs_sig))
    p, q = FS // g, int(fs_sig) // g
    fc = 1.0 / (2 * max(p, q))
    half = int(math.ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return p, q, h / np.sum(h)


def resample(x, fs_sig):
    if fs_sig == FS:
        return np.asarray(x, np.float64)
    p, q, h = resample_taps(fs_sig)
    return scipy.signal.resample_poly(np.asarray(x, np.float64), p, q, window=h)


def polyphase(x, fs_sig):
    """The polyphase statement of resample_poly the kernel implements: out[m] = p sum_i h[m q + L - p i] x[i]."""
    p, q, h = resample_taps(fs_sig)
    x = np.asarray(x, np.float64)
    n, half = len(x), (len(h) - 1) // 2
    out = np.zeros(-(-n * p // q))
    for m in range(len(out)):
        c = m * q + half
        i = np.arange(max(0, -(-(c - 2 * half) // p)), min(n - 1, c // p) + 1)
        out[m] = p * np.sum(h[c - p * i] * x[i])
    return out


def band_table():
    """-> (first bin, one past the last bin) of the 15 third-octave bands on the grid k 10000 / 512."""
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    k = np.arange(NUMBAND)
    lo = np.array([int(np.argmin((f - MINFREQ * 2.0 ** ((2 * i - 1) / 6)) ** 2)) for i in k])
    hi = np.array([int(np.argmin((f - MINFREQ * 2.0 ** ((2 * i + 1) / 6)) ** 2)) for i in k])
    return lo, hi


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


class Yard:
    """What the yardstick returns: d, status (0 scored, 1 T < 30, 2 no frame), n_kept, T, the keep-threshold margin in dB and the kept frames."""

    def __init__(self, d, status, n_kept, T, margin, kept):
        self.d, self.status, self.n_kept, self.T, self.margin, self.kept = d, status, n_kept, T, margin, kept


def _keep(x10):
    w = window()
    starts = list(range(0, len(x10) - N_FRAME, HOP))
    if not starts:
        return starts, [], np.inf
    E = np.array([20 * np.log10(np.linalg.norm(w * np.asarray(x10[i:i + N_FRAME], np.float64)) + EPS) for i in starts])
    thr = np.max(E) - DYN_RANGE
    return starts, [f for f in range(len(starts)) if E[f] > thr], float(np.min(np.abs(E - thr)))


def _segments_loop(X, Y):
    """Step 5 in float64, by loops: X, Y (15, T) -> d."""
    T = X.shape[1]
    clip = 1 + 10 ** (-BETA / 20)
    total = 0.0
    for m in range(N_SEG, T + 1):
        for b in range(NUMBAND):
            xs, ys = X[b, m - N_SEG:m].astype(np.float64), Y[b, m - N_SEG:m].astype(np.float64)
            c = np.sqrt(np.sum(xs * xs)) / (np.sqrt(np.sum(ys * ys)) + EPS)
            yp = np.minimum(c * ys, xs * clip)
            yp = yp - np.mean(yp)
            xs = xs - np.mean(xs)
            yp = yp / (np.sqrt(np.sum(yp * yp)) + EPS)
            xs = xs / (np.sqrt(np.sum(xs * xs)) + EPS)
            total += float(np.sum(yp * xs))
    return total / ((T - N_SEG + 1) * NUMBAND)


def stoi_yardstick(x, y, fs_sig):
    """The float64 yardstick, straight from the definition."""
    x10, y10 = resample(x, fs_sig), resample(y, fs_sig)
    w = window()
    starts, kept, margin = _keep(x10)
    if not starts:
        return Yard(np.nan, 2, 0, -1, margin, kept)
    nk = len(kept)
    xs, ys = np.zeros((nk - 1) * HOP + N_FRAME), np.zeros((nk - 1) * HOP + N_FRAME)
    for k, f in enumerate(kept):
        i = starts[f]
        xs[k * HOP:k * HOP + N_FRAME] += w * x10[i:i + N_FRAME]
        ys[k * HOP:k * HOP + N_FRAME] += w * y10[i:i + N_FRAME]
    lo, hi = band_table()
    fr = list(range(0, len(xs) - N_FRAME, HOP))
    T = len(fr)
    X, Y = np.zeros((NUMBAND, T)), np.zeros((NUMBAND, T))
    for t, i in enumerate(fr):
        sx, sy = np.fft.rfft(w * xs[i:i + N_FRAME], NFFT), np.fft.rfft(w * ys[i:i + N_FRAME], NFFT)
        for b in range(NUMBAND):
            X[b, t] = np.sqrt(np.sum(np.abs(sx[lo[b]:hi[b]]) ** 2))
            Y[b, t] = np.sqrt(np.sum(np.abs(sy[lo[b]:hi[b]]) ** 2))
    if T < N_SEG:
        return Yard(1e-5, 1, nk, T, margin, kept)
    return Yard(_segments_loop(X, Y), 0, nk, T, margin, kept)


def _segments_vec(X, Y):
    T = X.shape[1]
    idx = np.arange(N_SEG)[None, :] + np.arange(T - N_SEG + 1)[:, None]
    xs, ys = X[:, idx].astype(np.float64), Y[:, idx].astype(np.float64)                   # (15, J, 30)
    nrm = lambda a: np.sqrt(np.sum(a * a, axis=-1, keepdims=True))
    yp = np.minimum(ys * (nrm(xs) / (nrm(ys) + EPS)), xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - np.mean(yp, axis=-1, keepdims=True)
    xs = xs - np.mean(xs, axis=-1, keepdims=True)
    return float(np.sum((yp / (nrm(yp) + EPS)) * (xs / (nrm(xs) + EPS))) / (idx.shape[0] * NUMBAND))


def _staged(x, y, fs_sig, dt):
    """Whole-array form; dt = float64: the yardstick's arithmetic; float32: the kernels' staging."""
    x10, y10 = resample(x, fs_sig).astype(dt), resample(y, fs_sig).astype(dt)
    w = window().astype(dt)
    starts, kept, margin = _keep(x10)
    if not starts:
        return Yard(np.nan, 2, 0, -1, margin, kept)
    nk = len(kept)
    sel = np.array(starts)[kept][:, None] + np.arange(N_FRAME)[None, :]
    ola = []
    for s in (x10, y10):
        fr = w * s[sel]                                                                  # (nk, 256)
        o = np.zeros((nk + 1, HOP), dt)
        o[:-1] += fr[:, :HOP]
        o[1:] += fr[:, HOP:]
        ola.append(o.reshape(-1))
    T = nk - 1
    lo, hi = band_table()
    tob = []
    for o in ola:
        fr = w * o[(np.arange(T) * HOP)[:, None] + np.arange(N_FRAME)[None, :]] if T > 0 else np.zeros((0, N_FRAME), dt)
        sp = scipy.fft.rfft(fr, NFFT, axis=-1)
        assert sp.dtype == (np.complex64 if dt == np.float32 else np.complex128)
        pw = sp.real * sp.real + sp.imag * sp.imag
        tob.append(np.sqrt(np.stack([np.sum(pw[:, lo[b]:hi[b]], axis=-1, dtype=dt) for b in range(NUMBAND)])))
    if T < N_SEG:
        return Yard(1e-5, 1, nk, T, margin, kept)
    return Yard(_segments_vec(tob[0], tob[1]), 0, nk, T, margin, kept)


def stoi_vectorised(x, y, fs_sig):
    return _staged(x, y, fs_sig, np.float64)


def stoi_f32_staged(x, y, fs_sig):
    return _staged(x, y, fs_sig, np.float32)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def speech_like(seed, n, fs_sig):
    """Band-passed noise (300-3400 Hz) with 4 Hz and 0.7 Hz amplitude modulation, one stretch of exact zeros and two stretches 50-70 dB
    down; float64, about 0.1 rms."""
    rng = np.random.default_rng(1000 + seed)
    sos = scipy.signal.butter(4, [300, min(3400, 0.45 * fs_sig)], btype='bandpass', fs=fs_sig, output='sos')
    t = np.arange(n) / fs_sig
    ph = rng.uniform(0, 2 * np.pi, 2)
    x = scipy.signal.sosfilt(sos, rng.standard_normal(n + 2000))[2000:]
    x = 0.15 * x * (0.55 + 0.45 * np.sin(2 * np.pi * 4 * t + ph[0])) * (0.7 + 0.3 * np.sin(2 * np.pi * 0.7 * t + ph[1]))
    a = lambda u: int(u * n)
    x[a(0.30):a(0.37)] = 0.0
    x[a(0.55):a(0.61)] *= 10 ** (-55 / 20)
    x[a(0.80):a(0.85)] *= 10 ** (-65 / 20)
    return x


@functools.lru_cache(maxsize=None)
def make_pair(seed, n, fs_sig, kind):
    """x speech-like, y = x + white noise at `kind` dB SNR, or kind = 'filt': x through a short FIR.  float32, read-only."""
    x = speech_like(seed, n, fs_sig)
    rng = np.random.default_rng(2000 + seed)
    if kind == 'filt':
        y = scipy.signal.lfilter([1.0, 0.0, 0.0, -0.6, 0.0, 0.3, 0.0, 0.0, 0.0, 0.2], [1.0], x)
    else:
        v = rng.standard_normal(n)
        y = x + v * np.sqrt(np.mean(x * x) / np.mean(v * v) / 10 ** (kind / 10))
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def yard_of(seed, n, fs_sig, kind, vectorised=False):
    x, y = make_pair(seed, n, fs_sig, kind)
    return (stoi_vectorised if vectorised else stoi_yardstick)(x, y, fs_sig)


def compared_cases():
    return [(fs, n, seed, snr) for fs, n in CASES for seed in SEEDS for snr in SNRS]


def assert_precondition(yd, what):
    """Asserted, not skipped: the keep decision is not on a knife's edge and d is in the range where STOI discriminates."""
    assert yd.status == 0, (what, yd.status)
    assert yd.margin >= 0.01, (what, 'keep-threshold margin', yd.margin)
    assert 0.3 < yd.d < 0.999, (what, 'd', yd.d)


# ---- checks through the library ------------------------------------------------------------------------------------------------
def _eng():
    from disco_amd import metrics as dm
    return dm._engine()


def check_against_yardstick(fs_sig, n):
    """All seeds and SNRs of one (fs, n) in one batch, through Engine.stoi and metrics.stoi."""
    from disco_amd import metrics as dm
    keys = [(seed, snr) for seed in SEEDS for snr in SNRS]
    x = np.stack([make_pair(seed, n, fs_sig, snr)[0] for seed, snr in keys])
    y = np.stack([make_pair(seed, n, fs_sig, snr)[1] for seed, snr in keys])
    d, status, kept = _eng().stoi(x, y, fs_sig, want_kept=True)
    d2 = dm.stoi(x.reshape(3, 3, n), y.reshape(3, 3, n), fs_sig)
    assert d2.shape == (3, 3) and np.array_equal(d2.reshape(-1), d)
    worst = 0.0
    for i, (seed, snr) in enumerate(keys):
        yd = yard_of(seed, n, fs_sig, snr)
        assert_precondition(yd, (fs_sig, n, seed, snr))
        err = abs(d[i] - yd.d)
        worst = max(worst, err)
        print(f'fs {fs_sig} n {n} seed {seed} snr {snr:+.0f}: d {d[i]:.9f} yardstick {yd.d:.9f} |err| {err:.3g} kept {kept[i]}/{len(yd.kept)} margin {yd.margin:.3g} dB')
        assert status[i] == 0 and kept[i] == yd.n_kept
        assert err < TOL_STOI, (fs_sig, n, seed, snr, d[i], yd.d)
    print(f'fs {fs_sig} n {n}: worst |err| = {worst:.3g} (TOL_STOI {TOL_STOI:g})')


def edge_signal(n10, zero=(), burst=None, seed=7):
    """A 10-kHz pair of n10 samples: x modulated noise with the sample ranges `zero` set to exact zero and, with `burst`, eight strong
    samples at that position; y = x + white noise at 5 dB."""
    rng = np.random.default_rng(3000 + seed)
    t = np.arange(n10) / FS
    x = 0.1 * rng.standard_normal(n10) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    for a, b in zero:
        x[a:b] = 0.0
    if burst is not None:
        x[burst:burst + 8] = 0.3 * np.sign(rng.standard_normal(8))
    v = rng.standard_normal(n10)
    y = x + v * np.sqrt(np.mean(x * x) / np.mean(v * v) / 10 ** 0.5)
    return x.astype(np.float32), y.astype(np.float32)


def edge_cases():
    """name -> (x, y, expectation on the yardstick's kept frames as a function of the frame count NF)."""
    full = lambda NF: list(range(NF))
    c = {}
    for T in (29, 30, 31):                                                               # no frame removed: T = NF - 1
        c[f'T{T}'] = edge_signal(N_FRAME + HOP * (T + 1) - 5) + (full,)
    for dlt in (-1, 0, 1):                                                               # (n10 - 256) a multiple of 128, and that +- 1
        c[f'mult128{dlt:+d}'] = edge_signal(N_FRAME + HOP * 40 + dlt) + (full,)
    n10 = N_FRAME + HOP * 45 - 60                                                        # 45 frames
    c['first_removed'] = edge_signal(n10, zero=((0, N_FRAME),)) + (lambda NF: list(range(1, NF)),)
    c['last_removed'] = edge_signal(n10, zero=((HOP * 44, n10),)) + (lambda NF: list(range(NF - 1)),)
    # frames 10 .. 13 and 15 .. 19 hold nothing but the feet of the window under a burst in the middle of frame 14
    c['single_kept'] = edge_signal(n10, zero=((HOP * 10, HOP * 19 + N_FRAME),), burst=HOP * 14 + HOP - 4) + \
        (lambda NF: list(range(10)) + [14] + list(range(20, NF)),)
    return c


def check_frame_count_edges():
    from disco_amd import metrics as dm
    for name, (x, y, want_kept) in edge_cases().items():
        yd = stoi_yardstick(x, y, FS)
        NF = len(range(0, len(x) - N_FRAME, HOP))
        assert yd.kept == want_kept(NF), (name, yd.kept)
        assert yd.margin >= 0.01, (name, yd.margin)
        d, status, kept = _eng().stoi(x[None], y[None], FS, want_kept=True)
        print(f'{name}: n10 {len(x)} frames {NF} kept {kept[0]} T {yd.T} d {d[0]:.9f} yardstick {yd.d:.9f} status {status[0]}')
        assert kept[0] == yd.n_kept and status[0] == yd.status
        if name == 'T29':
            assert yd.T == 29 and status[0] == 1 and d[0] == 1e-5
            with pytest.warns(RuntimeWarning):
                assert dm.stoi(x, y, FS) == 1e-5
        else:
            assert yd.T >= N_SEG and (name not in ('T30', 'T31') or yd.T == int(name[1:]))
            assert abs(d[0] - yd.d) < TOL_STOI, (name, d[0], yd.d)
            with warnings.catch_warnings():
                warnings.simplefilter('error')
                assert dm.stoi(x, y, FS) == d[0]
    # a span under 257 samples at 10 kHz: no frame at all
    x, y = edge_signal(2000)
    for fs_sig, n in ((FS, 256), (16000, 409), (FS, 1)):                                   # ceil(409 * 5 / 8) = 256
        d, status = _eng().stoi(x[None, :n], y[None, :n], fs_sig)
        assert status[0] == 2 and np.isnan(d[0]), (fs_sig, n, d, status)
        with pytest.raises(ValueError, match='pair'):
            dm.stoi(x[:n], y[:n], fs_sig)
    d, status = _eng().stoi(x[None, :410], y[None, :410], 16000)                          # 257 samples: one frame, T = 0
    assert status[0] == 1 and d[0] == 1e-5
    with pytest.raises(ValueError, match=r'pair \(1, 0\)'):
        dm.stoi(np.stack([x, x])[:, None], np.stack([y, y])[:, None], FS, stop=np.array([[2000], [100]]))
    with pytest.raises(NotImplementedError):
        dm.stoi(x, y, FS, extended=True)
    with pytest.raises(ValueError):
        dm.stoi(x, y[:-1], FS)


def check_all_zero_x():
    from disco_amd import metrics as dm
    _, y = make_pair(1, 16000, 16000, 5.0)
    for fs_sig in (16000, FS):
        d, status, kept = _eng().stoi(np.zeros((1, 16000), np.float32), y[None], fs_sig, want_kept=True)
        assert status[0] == 0 and d[0] == 0.0 and not np.isnan(d[0]), (d, status)
        assert kept[0] == len(range(0, (16000 * FS // fs_sig) - N_FRAME, HOP))            # equal energies: every frame kept
    assert dm.stoi(np.zeros(16000, np.float32), y, 16000) == 0.0
    yd = stoi_yardstick(np.zeros(16000, np.float32), y, 16000)
    assert yd.d == 0.0


def check_bit_identity(n=16003, fs_sig=16000):
    """Alone, in a batch of 24, in a batch walked under a tiny budget; per-pair stop against slices; start / stop against slicing."""
    eng = _eng()
    kinds = (20.0, 5.0, -5.0, 'filt')
    x = np.stack([make_pair(1 + i % 3, n, fs_sig, kinds[i % 4])[0] for i in range(24)])
    y = np.stack([make_pair(1 + i % 3, n, fs_sig, kinds[i % 4])[1] for i in range(24)])
    d, status = eng.stoi(x, y, fs_sig)
    assert np.all(status == 0) and len(set(d.tolist())) == 12
    assert np.array_equal(d[:6], eng.stoi(x[:6], y[:6], fs_sig)[0])                        # run to run, and a smaller batch
    for i in (7, 23):
        assert eng.stoi(x[i:i + 1], y[i:i + 1], fs_sig)[0][0] == d[i], i
    per_pair = eng.lib.disco_stoi_workspace_bytes(eng.ctx, 1, n, 5, 8, 581)
    d5, st5 = eng.stoi(x, y, fs_sig, budget_bytes=5 * per_pair + 4096)                     # chunks of 5, 5, 5, 5, 4
    assert np.array_equal(d5, d) and np.array_equal(st5, status)
    d1, st1 = eng.stoi(x[:3], y[:3], fs_sig, budget_bytes=1)                               # one pair per call
    assert np.array_equal(d1, d[:3]) and np.array_equal(st1, status[:3])
    # per-pair stop: every pair as if sliced and scored alone
    start = 37
    stops = np.array([n - 13 * i for i in range(24)])
    stops[5] = start + 300                                                                 # too short for a frame
    stops[6] = start + 3000                                                                # a dozen frames: 1e-5
    dp, sp = eng.stoi(x, y, fs_sig, start=start, stop=stops)
    for i in (0, 5, 6, 11, 23):
        da, sa = eng.stoi(np.ascontiguousarray(x[i:i + 1, start:stops[i]]), np.ascontiguousarray(y[i:i + 1, start:stops[i]]), fs_sig)
        assert sa[0] == sp[i] and (da[0] == dp[i] or (np.isnan(da[0]) and np.isnan(dp[i]))), (i, da, dp[i])
    assert sp[5] == 2 and sp[6] == 1 and dp[6] == 1e-5 and np.all(np.delete(sp, (5, 6)) == 0)
    # scalar start / stop equals slicing; at 10 kHz too (no resampled copy: the kernels read the caller's rows from `start`)
    for fs2 in (fs_sig, FS):
        ds, ss = eng.stoi(x[:4], y[:4], fs2, start=101, stop=n - 55)
        dsl, ssl = eng.stoi(np.ascontiguousarray(x[:4, 101:n - 55]), np.ascontiguousarray(y[:4, 101:n - 55]), fs2)
        assert np.array_equal(ds, dsl) and np.array_equal(ss, ssl) and np.all(ss == 0)
    with pytest.raises(ValueError):
        eng.stoi(x, y, fs_sig, start=5, stop=n + 1)
    with pytest.raises(ValueError):
        eng.stoi(x, y[:, :-1], fs_sig)


def check_device_resident(n=9603, fs_sig=16000):
    """Device-resident inputs are read in place, chunked or not: the same bits as the NumPy route."""
    import torch
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    x = np.stack([make_pair(1 + i % 3, n, fs_sig, 5.0)[0] for i in range(6)])
    y = np.stack([make_pair(1 + i % 3, n, fs_sig, 5.0)[1] for i in range(6)])
    eng = _eng()
    d, _ = eng.stoi(x, y, fs_sig)
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    assert np.array_equal(eng.stoi(tx, ty, fs_sig)[0], d)
    assert np.array_equal(eng.stoi(tx, ty, fs_sig, budget_bytes=1)[0], d)


def stoi_room(K=2, fs=16000, L=16000 + 16000, seed=5):
    """K speech-like nodes with their dry sources, shaped like bss_checks.room_signals."""
    rng = np.random.default_rng(seed)
    s_dry = speech_like(seed, L, fs)
    n_dry = 0.05 * rng.standard_normal(L)
    s_in = np.stack([scipy.signal.lfilter(np.r_[np.zeros(3 + 2 * k), 0.8, 0.3 * rng.standard_normal(40) * np.exp(-np.arange(40) / 12)], [1.0], s_dry) for k in range(K)])
    n_in = np.stack([scipy.signal.lfilter(np.r_[0.7, 0.2 * rng.standard_normal(30)], [1.0], n_dry) for k in range(K)])
    sf_t, nf_t = 0.9 * s_in + 0.002 * rng.standard_normal((K, L)), 0.3 * n_in
    szf_t, nzf_t = 0.8 * s_in + 0.004 * rng.standard_normal((K, L)), 0.6 * n_in
    d = dict(s_in=s_in, n_in=n_in, sf_t=sf_t, nf_t=nf_t, szf_t=szf_t, nzf_t=nzf_t, s_dry=s_dry, n_dry=n_dry, y_in=s_in + n_in,
             sh_t=sf_t + nf_t, szh_t=szf_t + nzf_t)
    return {k: np.asarray(v, np.float32) for k, v in d.items()}


def check_room_results(tmp_path, fs=16000):
    from disco_amd.speech_enhancement import results_io as rio
    g = stoi_room()
    K = g['s_in'].shape[0]
    kw = dict(rnd_snrs=[3.0], fs=fs)
    pos = [g[k] for k in ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')]
    times = dict(y_in=g['y_in'], sh_t=g['sh_t'], szh_t=g['szh_t'])
    assert rio.STOI_KEYS == ('delta_stoi_cnv', 'delta_stoi', 'delta_stoi_dry') and not set(rio.STOI_KEYS) & set(rio.BSS_KEYS)
    res, resz = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], bss_flen=8, stoi=True, **times, **kw)
    assert tuple(res) == rio.RESULT_KEYS_TANGO and tuple(resz) == rio.RESULT_KEYS_MWF
    assert 'delta_stoi' not in res and 'delta_stoi_cnv' not in resz
    yd = lambda a, b: stoi_yardstick(a[fs:], b[fs:], fs)
    for k in range(K):
        s, dry = g['s_in'][k], g['s_dry']
        y_in = {c: yd(x, g['y_in'][k]) for c, x in (('cnv', s), ('dry', dry))}
        for c, x in (('cnv', s), ('dry', dry)):
            for r, key, est in ((res, 'delta_stoi_cnv' if c == 'cnv' else 'delta_stoi_dry', g['sh_t'][k]),
                                (resz, 'delta_stoi' if c == 'cnv' else 'delta_stoi_dry', g['szh_t'][k])):
                out = yd(x, est)
                assert out.status == 0 and y_in[c].status == 0 and min(out.margin, y_in[c].margin) >= 0.01
                want = out.d - y_in[c].d
                print(f'node {k} {key} ({"res" if r is res else "resz"}): {r[key][k]:.9f} yardstick {want:.9f}')
                assert abs(r[key][k] - want) < 2 * TOL_STOI, (key, k, r[key][k], want)
    assert res['delta_stoi_dry'] is not resz['delta_stoi_dry'] and not np.array_equal(res['delta_stoi_dry'], resz['delta_stoi_dry'])
    assert not np.array_equal(res['delta_stoi_cnv'], resz['delta_stoi'])
    for r in (res, resz):
        for key in rio.STOI_KEYS:
            assert key not in r or (r[key].shape == (K,) and np.all(np.isfinite(r[key]))), key
    # the other keys are what they are without stoi; stoi=False (the default) leaves NaN; without the dry sources the _dry key stays NaN
    r0, rz0 = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], bss_flen=8, **times, **kw)
    for r, rr in ((res, r0), (resz, rz0)):
        for key in r:
            if key in rio.STOI_KEYS:
                assert np.all(np.isnan(rr[key])), key
            else:
                assert np.array_equal(np.asarray(r[key]), np.asarray(rr[key]), equal_nan=True), key
    r1, rz1 = rio.room_results(*pos, bss_flen=8, stoi=True, **times, **kw)
    assert np.array_equal(r1['delta_stoi_cnv'], res['delta_stoi_cnv']) and np.array_equal(rz1['delta_stoi'], resz['delta_stoi'])
    assert np.all(np.isnan(r1['delta_stoi_dry'])) and np.all(np.isnan(rz1['delta_stoi_dry']))
    r2, rz2 = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], stoi=True, **kw)       # no time signals: nothing to score
    assert all(np.all(np.isnan(r[key])) for r in (r2, rz2) for key in rio.STOI_KEYS if key in r)
    files = rio.write_result_pickles(str(tmp_path), 11001, 'ssn', res, resz)
    for f, r in zip(files, (res, resz)):
        back = pickle.load(open(f, 'rb'))
        assert set(back) == set(r)
        for key in rio.STOI_KEYS:
            assert key not in r or np.array_equal(back[key], r[key])


def check_real_span(n=144000, fs_sig=16000, n_pair=24):
    """The span the reference scores (9 s at 16 kHz) as room_results issues it for one room of 4 nodes: 24 pairs in one call."""
    keys = [(1 + i % 3, SNRS[(i // 3) % 3]) for i in range(n_pair)]
    x = np.stack([make_pair(seed, n, fs_sig, snr)[0] for seed, snr in keys])
    y = np.stack([make_pair(seed, n, fs_sig, snr)[1] for seed, snr in keys])
    d, status, kept = _eng().stoi(x, y, fs_sig, want_kept=True)
    worst = 0.0
    for i, (seed, snr) in enumerate(keys):
        yd = yard_of(seed, n, fs_sig, snr, vectorised=i >= 2)           # the loops on two pairs, their whole-array form (test_stoi_cpu.py) on the rest
        assert_precondition(yd, (seed, snr))
        worst = max(worst, abs(d[i] - yd.d))
        assert status[i] == 0 and kept[i] == yd.n_kept and abs(d[i] - yd.d) < TOL_STOI, (seed, snr, d[i], yd.d)
    print(f'{n_pair} pairs of {n} samples: worst |err| = {worst:.3g}; d', d[:9])


def check_c3_room_through_the_path(fs=16000):
    """offline_tango -> iSTFT -> room_results(stoi=True) on one C3-shaped room: the keys finite and equal to metrics.stoi called directly."""
    import bss_checks as bc
    from disco_amd import metrics as dm
    from disco_amd.math_utils import my_istft
    from disco_amd.speech_enhancement import results_io as rio
    from disco_amd.speech_enhancement.tango import offline_tango
    y, s, n, s_dry, n_dry = bc.make_c3_room()
    K, M, L = y.shape
    yf, sf, nf, z_y, z_s, z_n = offline_tango(list(y), list(s), list(n), vads=['irm1', 'irm1'])[:6]
    t = lambda spec: np.stack([my_istft(spec[k], L) for k in range(K)])
    sh_t, sf_t, nf_t, szh_t, szf_t, nzf_t = t(yf), t(sf), t(nf), t(z_y), t(z_s), t(z_n)
    res, resz = rio.room_results(s[:, 0], n[:, 0], sf_t, nf_t, szf_t, nzf_t, rnd_snrs=[0.0], s_dry=s_dry, n_dry=n_dry, fs=fs,
                                 y_in=y[:, 0], sh_t=sh_t, szh_t=szh_t, bss_flen=8, stoi=True)
    for r in (res, resz):
        for key in rio.STOI_KEYS:
            assert key not in r or (r[key].shape == (K,) and np.all(np.isfinite(r[key]))), (key, r[key])
    cut = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)[..., fs:L])
    for k in range(K):
        d_in, d_out, d_z = (dm.stoi(cut(s[k, 0]), cut(e), fs) for e in (y[k, 0], sh_t[k], szh_t[k]))
        assert res['delta_stoi_cnv'][k] == d_out - d_in and resz['delta_stoi'][k] == d_z - d_in
        e_in, e_out, e_z = (dm.stoi(cut(s_dry), cut(e), fs) for e in (y[k, 0], sh_t[k], szh_t[k]))
        assert res['delta_stoi_dry'][k] == e_out - e_in and resz['delta_stoi_dry'][k] == e_z - e_in
    print('C3-shaped room through the path: delta_stoi_cnv', res['delta_stoi_cnv'], 'delta_stoi (step 1)', resz['delta_stoi'],
          'delta_stoi_dry', res['delta_stoi_dry'], resz['delta_stoi_dry'])
