"""Checks of the dry sources prepared on the device: the long real transform with random phases (csrc/k_sources.h k_src_wave_pass,
k_src_small_pass, k_src_mid: disco_noise_from_signal), the subtract-scale-shift-wrap pass (k_affine_segment: disco_affine_segment), and the
Python surface built on them (disco_amd.math_utils.next_pow_2, disco_amd.sigproc_utils.noise_from_signal,
disco_amd.dataset_utils.target_segments / noise_segments / ssn_segments).

Shared by tests/test_gpu_sources.py (real MI355X, `-m gpu`), tests/test_sources_emulated.py (the same kernel sources under the hipemu CPU
emulator) and tests/test_sources_cpu.py (the reference side alone: the conditions on the inputs).  `make_engine(**cfg)` builds a
disco_amd.engine.Engine bound to the library under test; the checks of the package-level functions use the package's own engine (the
emulated tier binds it to the emulator).

References and bars, none taken from a kernel's output:
  noise      `restate`, the float64 NumPy statement (rfft, abs * exp(2 pi i u), irfft, cut) that tests/golden/make_golden_sources.py found
             equal to the reference's noise_from_signal bit for bit, on the float32-rounded inputs.  Two figures, the relative L2 error and
             the largest absolute error over the output's rms; each must be <= NOISE_FACTOR = 4 times the same figure of `torch_route`, a
             float32 torch.fft.rfft / irfft run on the CPU on the same inputs: two correct float32 transforms differ in factorisation and
             twiddle rounding by a small factor either way, a wrong twiddle, stride or bin is off by orders of magnitude.
  placement  a cosine on bin k0 turned by a quarter: within PLACE_TOL = 1e-3 of the amplitude -- above the worst float32 error of a 2^22
             point transform (some 1e-5), three orders below a misplaced bin.
  affine     bit equality with np.float32((x.astype(float64) - mean) * gain).
  levels     max |out - ref| / max |ref| <= GAIN_TOL = 3e-5, derived in tests/roomsynth_checks.py; the VAD sample-exact, meaningful because
             tests/test_sources_cpu.py holds min |x2 - thr_| / thr_ >= 2e-4 on the reference side before and after the scaling.
"""
import functools
import os

import numpy as np

from roomsynth_checks import GAIN_TOL, ROOM_KW, _same_bits, room_scene, vad_margin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NOISE_FACTOR, PLACE_TOL = 4.0, 1e-3
ALL_P = tuple(range(10, 23))
# the smallest p of every pass plan (csrc/k_sources.h src_plan; W = a wave pass of 512 or 1024 points, s = a register pass of 4, 8 or 16):
#   10 [512]  11 [1024]  12 [512, s]  15 [1024, s]  16 [512, s, s]  19 [512, 512]  20 [512, 1024]  21 [1024, 1024]  22 [512, 512, s]
PLAN_P = (10, 11, 12, 15, 16, 19, 20, 21, 22)
PLACE_K0 = (1, 511, 512, 513, 1023, 1024, 1025)                  # ... and n_fft / 2 - 1
AFFINE_L = (1, 3, 4, 255, 256, 257)
AFFINE_LEAD = (0, 1, 4, 16000)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, 'sources_ref.npz')))


def _small_engine(make_engine):
    return make_engine(rooms=1, nodes=1, mics=1, length=1024)


def _package_engine():
    from disco_amd._engines import get_engine
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)


# ---- the reference side ------------------------------------------------------------------------------------------------------------------
def next_pow_2_reference(x):
    """math_utils.py:165."""
    return int(pow(2, np.ceil(np.log2(x))))


def restate(x, u, n_fft):
    """noise_from_signal with the phases given, in float64: x (L,), u (n_fft / 2 + 1,) in turns -> (L,)."""
    X = np.fft.rfft(np.asarray(x, np.float64), n_fft)
    return np.fft.irfft(np.abs(X) * np.exp(2j * np.pi * np.asarray(u, np.float64)), n_fft)[:len(x)]


def torch_route(x, u, n_fft):
    """The same three lines in float32 through torch.fft on the CPU: the yardstick of the bar, not the code under test."""
    import torch
    X = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(x, np.float32)), n=n_fft)
    ang = torch.from_numpy(np.ascontiguousarray(u, np.float32)) * np.float32(2 * np.pi)
    return torch.fft.irfft(torch.polar(X.abs(), ang), n=n_fft)[:len(x)].numpy()


def figures(got, ref):
    """(relative L2 error, largest absolute error over the rms of the reference)."""
    d = np.asarray(got, np.float64) - ref
    return float(np.linalg.norm(d) / np.linalg.norm(ref)), float(np.abs(d).max() / np.sqrt(np.mean(ref ** 2)))


def coloured(L, seed):
    """Coloured noise of amplitude ~ 0.1, float32."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(L + 2)
    x = w[2:] + 0.8 * w[1:-1] + 0.3 * w[:-2]
    return (0.1 * x / np.std(x)).astype(np.float32)


def phases(n, seed):
    return np.random.default_rng(seed).random(n).astype(np.float32)


def _hold_noise_bar(got, x, u, n_fft, what):
    ref = restate(x, u, n_fft)
    e, bar = figures(got, ref), figures(torch_route(x, u, n_fft), ref)
    print(f'sources noise {what}: rel L2 {e[0]:.3e} (torch float32 {bar[0]:.3e}), max / rms {e[1]:.3e} (torch float32 {bar[1]:.3e})')
    assert e[0] <= NOISE_FACTOR * bar[0] and e[1] <= NOISE_FACTOR * bar[1], (what, e, bar)
    return e


def affine_reference(x, stop, start, count, mean, gain, lead, out_len):
    """disco_affine_segment in NumPy: x (n_sig, len) -> (n_sig, out_len)."""
    n_sig, length = x.shape
    out = np.zeros((n_sig, out_len), np.float32)
    per = lambda v, i, default: default if v is None else (v if np.ndim(v) == 0 else v[i])
    for i in range(n_sig):
        L = int(per(stop, i, length))
        if L == 0:
            continue
        cnt = min(int(per(count, i, L)), out_len - lead)
        t = np.arange(max(cnt, 0))
        src = x[i, :L].astype(np.float64)[(int(per(start, i, 0)) + t) % L]
        out[i, lead:lead + len(t)] = np.float32((src - float(per(mean, i, 0.0))) * float(per(gain, i, 1.0)))
    return out


# ---- the long transform ------------------------------------------------------------------------------------------------------------------
def check_noise_sizes(make_engine, p):
    """One n_fft: L = n_fft, n_fft / 2 + 1 and one in between, in one batch through a stop per signal (NaN beyond it)."""
    eng = _small_engine(make_engine)
    n = 1 << p
    Ls = (n, n // 2 + 1, 3 * n // 4 + 3)
    x = np.full((3, n), np.nan, np.float32)
    u = np.stack([phases(n // 2 + 1, 100 * p + i) for i in range(3)])
    for i, L in enumerate(Ls):
        x[i, :L] = coloured(L, 200 * p + i)
    got = eng.noise_from_signal(x, u, stop=np.array(Ls), n_fft=n)
    assert got.shape == (3, n) and got.dtype == np.float32
    worst = (0.0, 0.0)
    for i, L in enumerate(Ls):
        assert not got[i, L:].any(), f'p = {p}, L = {L}: non-zero beyond the signal'
        worst = tuple(max(a, b) for a, b in zip(worst, _hold_noise_bar(got[i, :L], x[i, :L], u[i], n, f'p = {p}, L = {L}')))
    return worst


def check_noise_placement(make_engine, p):
    """x = cos(2 pi k0 t / n_fft) with u[k0] = 0.25 must come out as cos(2 pi k0 t / n_fft + pi / 2): rounding cannot hide a wrong index."""
    eng = _small_engine(make_engine)
    n = 1 << p
    k0s = [k for k in PLACE_K0 if k < n // 2 - 1] + [n // 2 - 1]
    t = np.arange(n)
    x = np.stack([np.cos(2 * np.pi * ((k * t) % n) / n) for k in k0s]).astype(np.float32)
    u = np.zeros((len(k0s), n // 2 + 1), np.float32)
    u[np.arange(len(k0s)), k0s] = 0.25
    got = eng.noise_from_signal(x, u, n_fft=n)
    for i, k in enumerate(k0s):
        err = float(np.abs(got[i] - np.cos(2 * np.pi * ((k * t) % n) / n + np.pi / 2)).max())
        assert err <= PLACE_TOL, f'p = {p}, k0 = {k}: off by {err} of the amplitude'


def check_noise_dc_nyquist(make_engine):
    """Any phase on bins 0 and n_fft / 2 gives the output of the real part alone."""
    eng = _small_engine(make_engine)
    for p in (10, 12):
        n = 1 << p
        x = coloured(n, 31 + p) + np.float32(0.05)
        x[::2] += np.float32(0.03)                                               # energy on the Nyquist bin as well
        u = phases(n // 2 + 1, 32 + p)
        u[0], u[-1] = 0.3, 0.7
        got = eng.noise_from_signal(x[None], u[None], n_fft=n)[0]
        X = np.fft.rfft(x.astype(np.float64), n)
        Y = np.abs(X) * np.exp(2j * np.pi * u.astype(np.float64))
        assert abs(Y[0].imag) > 1e-3 * np.abs(Y).mean() and abs(Y[-1].imag) > 1e-3 * np.abs(Y).mean()
        Y[0], Y[-1] = Y[0].real, Y[-1].real
        ref = np.fft.irfft(Y, n)
        e, bar = figures(got, ref), figures(torch_route(x, u, n), ref)
        assert e[0] <= NOISE_FACTOR * bar[0] and e[1] <= NOISE_FACTOR * bar[1], (p, e, bar)
        # with the DC phase at zero the output moves: that bin's phase does enter, through its cosine alone
        u2 = u.copy()
        u2[0] = 0.0
        moved = eng.noise_from_signal(x[None], u2[None], n_fft=n)[0]
        assert figures(moved, ref)[1] > 10 * e[1], 'the DC phase has no effect on this input: the check is empty'


def check_noise_batch(make_engine):
    """A row's bits alone and inside a batch of 5; NaN beyond a stop and in another row; zeros beyond L_i; L_i == 0; len beyond n_fft."""
    eng = _small_engine(make_engine)
    n, length = 2048, 2600
    stops = np.array([2048, 1025, 0, 1500, 2048])
    x = np.full((5, length), np.nan, np.float32)
    for i, L in enumerate(stops):
        x[i, :L] = coloured(int(L), 40 + i) if L else 0
    u = np.stack([phases(n // 2 + 1, 50 + i) for i in range(5)])
    got = eng.noise_from_signal(x, u, stop=stops, n_fft=n)
    assert got.shape == (5, length) and np.isfinite(got).all()
    for i, L in enumerate(stops):
        assert not got[i, L:].any(), f'row {i}: non-zero beyond L = {L}'
        alone = eng.noise_from_signal(np.ascontiguousarray(x[i:i + 1, :max(L, 1)]), u[i:i + 1], stop=np.array([L]), n_fft=n)
        _same_bits(alone[0, :L], got[i, :L], f'row {i} alone and in the batch')
        if L:
            _hold_noise_bar(got[i, :L], x[i, :L], u[i], n, f'batch row {i}, L = {L}')
    poisoned = x.copy()
    poisoned[3, :1500] = np.nan
    again = eng.noise_from_signal(poisoned, u, stop=stops, n_fft=n)
    assert np.isnan(again[3, :1500]).all() and not again[3, 1500:].any()
    for i in (0, 1, 2, 4):
        _same_bits(again[i], got[i], f'row {i} beside a NaN row')


def check_noise_refusals(make_engine):
    """Each refusal writes nothing (a sentinel fill) and names its limit, through the C ABI itself."""
    from disco_amd import _lib
    eng = _small_engine(make_engine)
    L = 1024
    px, kx = eng.to_device(coloured(L, 60)[None], np.float32)
    pu, ku = eng.to_device(phases(513, 61)[None], np.float32)
    sentinel = np.full((1, L), -7.0, np.float32)
    po, ko = eng.to_device(sentinel, np.float32)
    pstop, kstop = eng.to_device(np.array([400], np.int32), np.int32)
    call = lambda n_fft=1024, x=px, phase=pu, out=po, n_sig=1, stop=None, length=L: eng.lib.disco_noise_from_signal(
        eng.ctx, x, n_sig, length, stop, n_fft, phase, out, eng.stream)
    for n_fft in (1 << 9, 1 << 23):
        assert call(n_fft=n_fft, stop=pstop) == _lib.E_UNSUPPORTED, n_fft
        msg = eng.lib.disco_last_error(eng.ctx)
        assert b'2^10' in msg and b'2^22' in msg, msg
    for kw in (dict(n_fft=1000), dict(n_fft=0), dict(n_fft=-1024), dict(x=None), dict(phase=None), dict(out=None), dict(n_sig=-1)):
        assert call(**kw) == _lib.E_ARG, kw
    assert call(n_fft=1000) == _lib.E_ARG and b'power of two' in eng.lib.disco_last_error(eng.ctx)
    assert call(n_fft=1024, length=1025) == _lib.E_ARG and b'n_fft < len' in eng.lib.disco_last_error(eng.ctx)
    eng.sync()
    _same_bits(ko.numpy(), sentinel, 'out after the refusals')
    assert call() == 0                                                       # ... and the same buffers are then taken
    assert np.abs(ko.numpy()).max() < 1.0

    def refused(fn, text):
        try:
            fn()
        except ValueError as e:
            assert text in str(e), (text, str(e))
        else:
            raise AssertionError(f'not refused: {text}')
    x = coloured(3000, 62)[None]
    refused(lambda: eng.noise_from_signal(x, phases(1025, 63)[None], n_fft=2048), 'does not fit')
    refused(lambda: eng.noise_from_signal(x, phases(1025, 63)[None], n_fft=3000), 'power of two')
    refused(lambda: eng.noise_from_signal(x, phases(1025, 63)[None], n_fft=4096), 'phase must be')


# ---- subtract, scale, shift, wrap --------------------------------------------------------------------------------------------------------
def check_affine_bits(make_engine):
    """Every L, lead, start and count of the issue, on both access routes (out_len a multiple of 4 with aligned rows, and not)."""
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(70)
    n_cases = 0
    for L in AFFINE_L:
        x = rng.standard_normal((3, L)).astype(np.float32)
        start = np.array([0, 1 % L, L - 1])
        mean, gain = rng.standard_normal(3), 10.0 ** rng.uniform(-1, 1, 3)
        for lead in AFFINE_LEAD:
            for count in (1, L, L + 3):
                for out_len in {lead + L + 3, (lead + L + 3 + 3) // 4 * 4, lead + max(L - 1, 1)}:      # room for all, aligned, cut short
                    got = eng.affine_segment(x, start=start, count=count, mean=mean, gain=gain, lead=lead, out_len=out_len)
                    _same_bits(got, affine_reference(x, None, start, count, mean, gain, lead, out_len),
                               f'L = {L}, lead = {lead}, count = {count}, out_len = {out_len}')
                    n_cases += 1
    assert n_cases >= 6 * 4 * 3 * 2
    # the aligned route with sources that are whole aligned quads (start - lead a multiple of 4), that are not, and that wrap
    x = rng.standard_normal((4, 256)).astype(np.float32)
    start, count = np.array([0, 4, 6, 252]), np.array([256, 256, 300, 259])
    for lead in (0, 4, 8):
        got = eng.affine_segment(x, start=start, count=count, mean=0.25, gain=3.0, lead=lead, out_len=320)
        _same_bits(got, affine_reference(x, None, start, count, 0.25, 3.0, lead, 320), f'aligned quads, lead = {lead}')


def check_affine_stops(make_engine):
    """A length per signal (0 included) with NaN beyond it, the defaults from NULLs, zeros outside the segment."""
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(71)
    stops = np.array([1, 3, 4, 255, 256, 257, 0, 260])
    x = np.full((len(stops), 260), np.nan, np.float32)
    for i, L in enumerate(stops):
        x[i, :L] = rng.standard_normal(L)
    for lead, out_len in ((0, 260), (5, 300), (4, 264)):
        got = eng.affine_segment(x, stop=stops, mean=0.5, gain=2.0, lead=lead, out_len=out_len)
        assert np.isfinite(got).all()
        _same_bits(got, affine_reference(x, stops, None, None, 0.5, 2.0, lead, out_len), f'stops, lead = {lead}')
        assert not got[6].any(), 'L_i == 0 gives zeros'
    plain = rng.standard_normal((3, 37)).astype(np.float32)
    _same_bits(eng.affine_segment(plain), plain, 'every default: a copy')
    shifted = eng.affine_segment(plain, lead=7, out_len=50)
    assert not shifted[:, :7].any() and not shifted[:, 44:].any()
    _same_bits(shifted[:, 7:44], plain, 'lead alone: a shifted copy between zeros')


def check_affine_many_rows(make_engine, n_sig=70000, L=4):
    """More rows than the grid has workgroups (65 536)."""
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(72)
    x = rng.standard_normal((n_sig, L)).astype(np.float32)
    mean, gain = rng.standard_normal(n_sig), rng.uniform(0.5, 2.0, n_sig)
    got = eng.affine_segment(x, mean=mean, gain=gain, start=1, lead=1, out_len=L + 2)
    want = np.zeros((n_sig, L + 2), np.float32)
    want[:, 1:L + 1] = np.float32((np.roll(x, -1, axis=1).astype(np.float64) - mean[:, None]) * gain[:, None])
    _same_bits(got, want, f'{n_sig} rows')


def check_affine_refusals(make_engine):
    from disco_amd import _lib
    eng = _small_engine(make_engine)
    L = 64
    px, kx = eng.to_device(np.ones((1, L), np.float32), np.float32)
    sentinel = np.full((1, L), -7.0, np.float32)
    po, ko = eng.to_device(sentinel, np.float32)
    call = lambda x=px, out=po, n_sig=1, lead=0, out_len=L: eng.lib.disco_affine_segment(eng.ctx, x, n_sig, L, None, None, None, None, None, lead,
                                                                                       out, out_len, eng.stream)
    for kw in (dict(lead=-1), dict(lead=L + 1), dict(x=None), dict(out=None), dict(n_sig=-1)):
        assert call(**kw) == _lib.E_ARG, kw
    assert call(lead=L + 1) == _lib.E_ARG and b'lead' in eng.lib.disco_last_error(eng.ctx)
    eng.sync()
    _same_bits(ko.numpy(), sentinel, 'out after the refusals')
    assert call(lead=L) == 0                                                  # lead == out_len: all zeros
    assert not ko.numpy().any()
    assert call() == 0
    _same_bits(ko.numpy(), np.ones((1, L), np.float32), 'the same buffers are then taken')


# ---- the surface -------------------------------------------------------------------------------------------------------------------------
def check_noise_package():
    """sigproc_utils.noise_from_signal: under a seed against the reference's own output; two n_fft groups in one call; the container rule."""
    from disco_amd import sigproc_utils as su
    from disco_amd.engine import DevBuf
    fx = fixture()
    for i in range(int(fx['n_noise'])):
        x, ref = fx[f'noise_x{i}'], fx[f'noise_y{i}']
        np.random.seed(int(fx['noise_seed'][i]))
        got = su.noise_from_signal(x)
        assert isinstance(got, np.ndarray) and got.shape == x.shape and got.dtype == np.float32
        n_fft = 2 * (len(fx[f'noise_u{i}']) - 1)
        e, bar = figures(got, ref), figures(torch_route(x, fx[f'noise_u{i}'], n_fft), ref)
        print(f'sources noise_from_signal under seed, L = {len(x)}: {e} (torch float32 {bar})')
        assert e[0] <= NOISE_FACTOR * bar[0] and e[1] <= NOISE_FACTOR * bar[1], (i, e, bar)
    # rows of 1500 and 5000 samples in one call: n_fft 2048 and 8192
    stops = np.array([1500, 5000, 1400])
    x = np.zeros((3, 5000), np.float32)
    for i, L in enumerate(stops):
        x[i, :L] = coloured(int(L), 80 + i)
    u = np.stack([phases(4097, 83 + i) for i in range(3)])
    got = su.noise_from_signal(x, stop=stops, phase=u)
    for i, L in enumerate(stops):
        n_fft = 2048 if L <= 2048 else 8192
        assert not got[i, L:].any()
        _hold_noise_bar(got[i, :L], x[i, :L], u[i, :n_fft // 2 + 1], n_fft, f'two groups, row {i}')
    dev = su.noise_from_signal(_package_engine().to_device(x, np.float32)[1], stop=stops, phase=u)
    assert isinstance(dev, DevBuf) and dev.shape == x.shape
    _same_bits(dev.numpy(), got, 'device in, DevBuf out')


def check_target_segments():
    """Against the reference's get_target_segment: signal within GAIN_TOL of the largest value, the VAD sample-exact, the rest exact."""
    from disco_amd.dataset_utils import target_segments
    from disco_amd.engine import DevBuf
    fx = fixture()
    fs = int(fx['fs'])
    res = target_segments(fx['target_x'], fx['target_len'], float(fx['var_tar']), tuple(fx['duration_range']), fs=fs)
    assert isinstance(res['signal'], DevBuf) and isinstance(res['vad'], DevBuf)
    want_s, want_v = fx['target_signal'], fx['target_vad'].astype(np.float32)
    assert res['signal'].shape == want_s.shape == res['vad'].shape
    assert np.array_equal(res['ok'], fx['target_ok']) and res['ok'].dtype == bool
    assert np.array_equal(res['lengths'], fx['target_out_len'])
    assert np.array_equal(res['duration'], fx['target_duration'])
    sig, vad = res['signal'].numpy(), res['vad'].numpy()
    e = float(np.abs(sig - want_s).max() / np.abs(want_s).max())
    print('sources target_segments, signal against the reference over its largest value:', e, 'gain', res['gain'])
    assert e <= GAIN_TOL, e
    bad = vad != want_v
    assert not bad.any(), f'{int(bad.sum())} VAD samples wrong, first at {tuple(np.argwhere(bad)[0])}'
    assert not sig[~res['ok']].any() and not vad[~res['ok']].any() and not sig[:, :fs].any() and not vad[:, :fs].any()
    for i in np.flatnonzero(res['ok']):
        voiced = sig[i].astype(np.float64)[vad[i] == 1]
        assert abs(np.var(voiced) / float(fx['var_tar']) - 1) < 1e-3, np.var(voiced)
    # no voiced sample: a constant has an all-zero VAD, the reference would divide by the variance of nothing
    flat = target_segments(np.full((1, 9000), 0.25, np.float32), [9000], 1e-3, (0.5, 1.0), fs=fs)
    assert not flat['ok'][0] and not flat['signal'].numpy().any() and flat['lengths'][0] == 0
    return res


def check_noise_segments():
    from disco_amd.dataset_utils import noise_segments
    from disco_amd.engine import DevBuf
    rng = np.random.default_rng(90)
    lens, start = np.array([5000, 4000, 1200, 3000]), np.array([0, 3999, 700, 2500])
    noise = np.full((4, 5000), np.nan, np.float32)
    for i, L in enumerate(lens):
        noise[i, :L] = 0.1 * rng.standard_normal(L) + 0.02
    got = noise_segments(noise, lens, start, duration=0.125, fs=16000)
    assert isinstance(got, DevBuf) and got.shape == (4, 2000)
    got = got.numpy()
    for i, L in enumerate(lens):
        sig = noise[i, :L].astype(np.float64)
        y = np.roll(sig, len(sig) - start[i])[:int(0.125 * 16000)]              # signal_setups.py:134-136
        y -= np.mean(y)
        e = float(np.abs(got[i, :len(y)] - y).max() / np.abs(y).max())
        assert e <= GAIN_TOL, (i, e)
        assert not got[i, len(y):].any()


def check_ssn_segments():
    from disco_amd.dataset_utils import ssn_segments
    from disco_amd.engine import DevBuf
    lens = np.array([6000, 9000])
    talk = np.zeros((2, 9000), np.float32)
    for i, L in enumerate(lens):
        talk[i, :L] = coloured(int(L), 95 + i)
    u = np.stack([phases(8193, 97 + i) for i in range(2)])
    got = ssn_segments(talk, lens, duration=0.25, fs=16000, phase=u)
    assert isinstance(got, DevBuf) and got.shape == (2, 4000)
    got = got.numpy()
    for i, L in enumerate(lens):
        n_fft = 8192 if L <= 8192 else 16384
        ref = restate(talk[i, :L], u[i, :n_fft // 2 + 1], n_fft)[:4000]
        e, bar = figures(got[i], ref), figures(torch_route(talk[i, :L], u[i, :n_fft // 2 + 1], n_fft)[:4000], ref)
        assert e[0] <= NOISE_FACTOR * bar[0] and e[1] <= NOISE_FACTOR * bar[1], (i, e, bar)


def check_chain(R=2, L=8192):
    """target_segments -> ssn_segments -> simulate_rooms -> mix_rooms -> offline_tango_batched, device-resident end to end (K = 2, M = 2).
    The segment stage runs at a nominal 2048 Hz so that one second of leading silence and the signal make 8192 samples."""
    from disco_amd.dataset_utils import mix_rooms, simulate_rooms, ssn_segments, target_segments
    from disco_amd.engine import DevBuf
    from disco_amd.speech_enhancement.tango import offline_tango_batched
    fx = fixture()
    fs_seg = 2048
    eng = _package_engine()
    dry = eng.to_device(np.ascontiguousarray(fx['target_x'][:R, :7000]), np.float32)[1]
    tar = target_segments(dry, [7000] * R, 1e-3, (1.0, (L - fs_seg) / fs_seg), fs=fs_seg)
    assert tar['ok'].all() and isinstance(tar['signal'], DevBuf) and tar['signal'].shape == (R, L) and tar['vad'].shape == (R, L)
    talk = eng.to_device(np.stack([coloured(9000, 110 + r) for r in range(R)]), np.float32)[1]
    np.random.seed(5)
    ssn = ssn_segments(talk, [9000] * R, duration=L / fs_seg, fs=fs_seg)
    assert isinstance(ssn, DevBuf) and ssn.shape == (R, L)
    dims, absorption, src, mic = room_scene(R)
    rooms = simulate_rooms(tar['signal'], ssn, dims, absorption, src, mic, (2, 2), 5.0, (-100.0, 100.0), -1.0, target_vad=tar['vad'], **ROOM_KW)
    assert isinstance(rooms['images'], DevBuf) and rooms['images'].shape == (2, R, 4, L)
    y, s, n = mix_rooms(rooms['images'][0], rooms['images'][1], np.array([5.0, 0.0])[:R], (2, 2))
    assert all(isinstance(a, DevBuf) and a.shape == (R, 2, 2, L) for a in (y, s, n))
    res = offline_tango_batched(y, s, n)
    T = 1 + L // 256
    assert res['yf'].shape == (R, 2, T, 257), res['yf'].shape
    for k, v in res.items():
        assert np.isfinite(v).all(), k
    assert np.abs(res['yf']).max() > 0 and np.isfinite(y.numpy()).all()
