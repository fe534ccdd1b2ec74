"""Checks of the kernels that feed the path and score it, value by value: the TF masks (csrc/k_stft.h tf_mask_value through k_tf_mask,
k_tf_mask_channel and k_mask_oracle<512 | 1024>), the 'ivad' mask (csrc/k_vad.h k_vad_mask) and the level statistics (csrc/k_metrics.h
k_pair_stats, k_band_stats<GATED>), through Engine.tf_mask / tango_reference / mask_oracle / mask_ivad / pair_stats / band_stats and
disco_amd.metrics.

Shared by tests/test_gpu_mask_metrics.py (real MI355X, `-m gpu`), tests/test_mask_metrics_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut to the smallest shapes) and tests/test_mask_metrics_cpu.py (the reference side alone: the constant behind
the oracle-mask bar, the conditions on the inputs).  `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library under
test.  Every reference is computed here from oracle/ (pinned to the reference's own outputs), NumPy and SciPy; no bar comes from a
kernel's output.

A. ELEMENTWISE MASKS.  Reference: oracle.mwf_oracle.tf_mask on the complex64 inputs, evaluated in float64 (`ref_mask64`; for 'iam' the
   sum S + N is formed in complex64 first, as the reference does, so both sides round the cancelling sum identically).  Bar, every
   element: relative error of the mask <= (10 p + 4) 2^-24 (`mask_bar`; 4 2^-24 for p = 0) -- 1-ulp sqrt and division, 1.5 ulp on
   the sum of squares halved by the root, one rounding per multiply, p-fold growth through the power.  Non-finite values: NaN and
   +-inf exactly where the float32 reference (tf_mask on complex64, no float64 cast) has them -- the overflow of xi to inf and
   inf / inf = NaN are the reference's own behaviour.  Where a magnitude leaves float32 (|S|, |N| or |S + N| beyond 3.4e38) the
   float32 reference's value is the reference; where the mask itself is below float32's normal range, the float32 reference within one
   denormal quantum per rounding.  'ibm': decisions equal in every element with |xi / thr - 1| above the relative bar,
   and equal to the float32 reference's where a magnitude left float32; planted exact ties must answer 1, as the reference does.
B. PER-CHANNEL MASKS of the whole path (k_tf_mask_channel): bit for bit Engine.tf_mask of the reference channel's spectra.
C. ORACLE MASKS FROM TIME SIGNALS.  Reference: oracle.stft_oracle.stft in complex128, then tf_mask.  Bar of a bin:
   |m - ref| <= C_ORACLE delta G + 4 2^-24 |ref|, delta = 2^-24 sqrt(n_fft) (|windowed s frame|_2 + |windowed n frame|_2) the
   rounding unit of one spectrum bin, G the first-order sensitivity of the mask to a perturbation delta of each magnitude (`_sens`;
   written without dividing by |S|, so silent bins stay finite, and with |S|^(p - 1) taken at |S| + C_ORACLE delta, so that a silent bin
   of a p >= 2 mask may hold the square of a rounding unit and not only an exact 0).  C_ORACLE is 4 x the worst ratio (err - 4 2^-24 |ref|)+ / (delta G) of a float32
   restatement (in `oracle_case`: scipy.fft.rfft on float32 frames, the mask in float32) over every case of `oracle_cases()`;
   tests/test_mask_metrics_cpu.py recomputes it and holds the constant below to it.  'ibm': decisions equal in every bin with
   |xi - thr| above 4 delta p xi (1/|S| + 1/|N|).
D. VAD MASK.  Reference: oracle.mwf_oracle.ivad_mask on the same float32 signal.  Bar: zero frames wrong, constant over frequency.
   A constant non-zero signal is NOT a test input: x - mean is then 0 or one rounding of the mean away from it, and whether every
   sample or none exceeds the threshold depends on the last bit of the mean.  The reference's float32 pairwise mean and an exactly
   rounded mean (the kernel's: float64 sum, rounded once) disagree there.
E. LEVEL STATISTICS.  Counts exact.  Pair sums against float64 NumPy to 8 2^-53 sum|terms| (the worst case of a tree sum of float64
   terms).  Band sums per band against a long-double run of the same direct-form-II-transposed recurrence (`lfilter_ld`); bar of a
   band: BAND_FACTOR = 4 x the worst relative distance of scipy.signal.lfilter in float64 from that run over the same signals (and, in
   the dense banks, over the neighbouring bands inside the band's own pass band: `_pooled`), floor
   1e-13 -- the 'ba' form is ill-conditioned in the low bands (SciPy itself is 5e-4 off in the 160 Hz band at 16 kHz), so a flat bar
   would be blind or false.  Relative distance of sum y^2: |sum - ref| / ref.  Of sum y: the band-pass output sums to nearly nothing, so
   the sum's own size is no scale, and whether SciPy's sample errors cancel in a sum is luck (with one signal per workgroup the worst is
   over three signals); its distance is sum |y_scipy - y| / sum |y|, which bounds what any summation order of SciPy's samples could
   give, and the kernel's |sum - ref| / sum |y| is held to 4 x that.
"""
import functools

import numpy as np
import scipy.fft
import scipy.signal

from oracle import metrics_oracle as meo
from oracle import mwf_oracle as mo
from oracle import stft_oracle as so

U = 2.0 ** -24
EPS = mo.EPS
FLT_MAX = float(np.finfo(np.float32).max)
NAMES = tuple(f'{k}{p}' for k in ('irm', 'iam', 'ibm') for p in range(10))
C_ORACLE = 0.419                # 4 x the float32 restatement's worst err / (delta G) (tests/test_mask_metrics_cpu.py recomputes it)
BAND_FACTOR = 4.0
BAND_FLOOR = 1e-13


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = _bits(a) != _bits(b)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}'


def _raises(fn, text):
    from disco_amd.engine import DiscoError
    try:
        fn()
    except DiscoError as e:
        assert text in str(e), (text, str(e))
        return
    raise AssertionError(f'not refused: expected "{text}"')


def _small_engine(make_engine, **cfg):
    return make_engine(rooms=1, nodes=1, mics=1, length=1024, **cfg)


# ---- A. elementwise masks -----------------------------------------------------------------------------------------------------------
def mask_bar(p):
    return (10 * p + 4) * U


def ref_mask64(S, N, kind, bin_thr=0.0):
    """tf_mask of the complex64 inputs in float64.  'iam': the oracle's line on the sum already formed in complex64."""
    S, N = np.asarray(S, np.complex64), np.asarray(N, np.complex64)
    with np.errstate(all='ignore'):
        if kind.startswith('iam'):
            return (np.abs(S.astype(np.complex128)) / np.abs((S + N).astype(np.complex128))) ** int(kind[3])
        return np.asarray(mo.tf_mask(S.astype(np.complex128), N.astype(np.complex128), kind, bin_thr), np.float64)


def ref_mask32(S, N, kind, bin_thr=0.0):
    """The reference as it runs: tf_mask on complex64, float32 throughout."""
    with np.errstate(all='ignore'):
        return np.asarray(mo.tf_mask(np.asarray(S, np.complex64), np.asarray(N, np.complex64), kind, bin_thr))


def _in_float32(S, N, kind):
    """Elements whose inputs are finite and whose magnitudes |S|, |N| (|S + N| for 'iam') do not overflow float32."""
    S, N = np.asarray(S, np.complex64), np.asarray(N, np.complex64)
    with np.errstate(all='ignore'):
        ok = np.isfinite(S) & np.isfinite(N) & (np.abs(S.astype(np.complex128)) <= FLT_MAX)
        other = (S + N) if kind.startswith('iam') else N
        return ok & np.isfinite(other) & (np.abs(other.astype(np.complex128)) <= FLT_MAX)


def compare_mask(m, S, N, kind, bin_thr=0.0, what=''):
    """Every element of m against the references of section A.  -> the worst err / bar over the elements held to the float64 reference
    ('ibm': the number of elements inside the band where either decision stands)."""
    m = np.asarray(m)
    p = int(kind[3])
    bar = mask_bar(p)
    r32, r64, inside = ref_mask32(S, N, kind, bin_thr), ref_mask64(S, N, kind, bin_thr), _in_float32(S, N, kind)
    assert m.shape == r64.shape, (what, m.shape, r64.shape)
    if kind.startswith('ibm'):
        assert np.all((m == 0) | (m == 1)), (what, kind, 'a decision is 0 or 1')
        with np.errstate(all='ignore'):
            xi = (np.abs(np.asarray(S, np.complex64).astype(np.complex128)) /
                  np.maximum(np.abs(np.asarray(N, np.complex64).astype(np.complex128)), EPS)) ** p
            clear = inside & ((np.abs(xi / 10 ** (bin_thr / 10) - 1) > bar) | (p == 0))      # p = 0: xi is 1 exactly on both sides
        bad = (clear & (m != r64)) | (~inside & (m != r32.astype(np.float32)))
        assert not bad.any(), f'{what} {kind} thr {bin_thr} dB: {int(bad.sum())} wrong decisions of {bad.size}, first at {np.argwhere(bad)[0]}'
        return int((inside & ~clear).sum())
    nan, inf = np.isnan(r32), np.isinf(r32)
    bad = (np.isnan(m) != nan) | (np.isinf(m) != inf) | (inf & (np.sign(m) != np.sign(r32)))
    assert not bad.any(), (f'{what} {kind}: {int(bad.sum())} of {bad.size} elements are NaN / inf where the float32 reference is not, or the '
                           f'reverse; first at {np.argwhere(bad)[0]}: got {m[tuple(np.argwhere(bad)[0])]}, reference {r32[tuple(np.argwhere(bad)[0])]}')
    fin = ~(nan | inf)
    # a mask below float32's normal range (xi^p underflows: |S| = 1e-38 over the EPS clamp, squared) lives on the denormal grid, outside the
    # derivation of the relative bar: there the float32 reference within one quantum 2^-149 per rounding (the division, p - 1 products)
    under = fin & inside & (np.abs(r64) < 2.0 ** -126)
    with np.errstate(invalid='ignore'):
        bad = under & (np.abs(m.astype(np.float64) - r32.astype(np.float64)) > max(p, 1) * 2.0 ** -149)
    assert not bad.any(), f'{what} {kind}: {int(bad.sum())} denormal masks more than {max(p, 1)} quanta from the float32 reference'
    fin &= ~under
    ref = np.where(inside, r64, r32.astype(np.float64))[fin]
    err = np.abs(m[fin].astype(np.float64) - ref)
    ratio = np.where(ref != 0, err / (bar * np.abs(np.where(ref != 0, ref, 1))), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f'{what} {kind}: worst relative error {worst * bar:.3g} = {worst:.3g} x the bar {bar:.3g}; {int((ratio > 1).sum())} of {ratio.size} elements beyond it'
    return worst


def _gauss(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def check_every_name(make_engine, n=3000):
    """All thirty accepted names on Gaussian elements; 'ibm' at three thresholds."""
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(11)
    S, N = _gauss(rng, n), _gauss(rng, n)
    out = {}
    for kind in NAMES:
        for thr in ((-6.0, 0.0, 3.0) if kind.startswith('ibm') else (0.0,)):
            out[kind if thr == 0 else f'{kind}@{thr:g}dB'] = compare_mask(eng.tf_mask(S, N, type=kind, bin_thr=thr).numpy(), S, N, kind, thr, 'every name')
    return {'irm': max(v for k, v in out.items() if k.startswith('irm')), 'iam': max(v for k, v in out.items() if k.startswith('iam')),
            'ibm_in_band': sum(v for k, v in out.items() if k.startswith('ibm'))}


def sweep_inputs(per_decade=500, seed=12):
    """|S| in two-decade steps from 1e-38 to 1e38, |N| / |S| within 1e+-2, random phases; the ends leave complex64 (inf, denormals)."""
    rng = np.random.default_rng(seed)
    mag = np.repeat(10.0 ** np.arange(-38, 39, 2), per_decade)
    S = mag * np.exp(2j * np.pi * rng.random(mag.size))
    N = mag * 10.0 ** rng.uniform(-2, 2, mag.size) * np.exp(2j * np.pi * rng.random(mag.size))
    with np.errstate(over='ignore'):
        return S.astype(np.complex64), N.astype(np.complex64), mag


def check_magnitude_sweep(make_engine, kinds=('irm1', 'irm2', 'iam1', 'ibm1'), per_decade=500):
    eng = _small_engine(make_engine)
    S, N, _ = sweep_inputs(per_decade)
    return {kind: compare_mask(eng.tf_mask(S, N, type=kind).numpy(), S, N, kind, 0.0, 'magnitude sweep') for kind in kinds}


def special_inputs():
    rng = np.random.default_rng(13)
    g, h = _gauss(rng, 64), _gauss(rng, 64)
    z = np.zeros(64, np.complex64)
    tiny = (h * np.float32(1e-18)).astype(np.complex64)                  # |N| below EPS: the clamp
    big = (g * np.float32(1e25)).astype(np.complex64)                    # xi overflows for p >= 2
    # |S|^2 or |N|^2 either side of 2^+-100, where tf_mask_value changes between its plain and its scaled route
    seam = lambda a, e: (a * np.float32(2.0 ** e) * rng.uniform(0.5, 2, 64).astype(np.float32)).astype(np.complex64)
    return {'S=0': (z, h), 'N=0': (g, z), 'both 0': (z, z), '|N| < EPS': (g, tiny), 'S = -N': (g, -g), 'xi overflows': (big, h),
            '|N| at the clamp': (g, np.full(64, EPS, np.complex64)), 'both at 2^50': (seam(g, 50), seam(h, 50)),
            'both at 2^-50': (seam(g, -50), seam(h, -50)), 'S at 2^50': (seam(g, 50), h), 'N at 2^-50': (g, seam(h, -50))}


def check_special_inputs(make_engine):
    eng = _small_engine(make_engine)
    for what, (S, N) in special_inputs().items():
        for kind in ('irm1', 'irm2', 'irm3', 'iam1', 'iam2', 'ibm1', 'ibm2', 'irm0', 'iam0', 'ibm0'):
            compare_mask(eng.tf_mask(S, N, type=kind).numpy(), S, N, kind, 0.0, what)


def tie_inputs(n=512, seed=14):
    """|S| and |N| bit-identical: N = S, -S, conj(S), i S, at unit scale and across the float32 range."""
    rng = np.random.default_rng(seed)
    S = (_gauss(rng, n) * (10.0 ** rng.integers(-12, 16, n)).astype(np.float32)).astype(np.complex64)      # |N| stays above the EPS clamp
    return {'N = S': (S, S.copy()), 'N = -S': (S, -S), 'N = conj(S)': (S, np.conj(S)), 'N = i S': (S, (S.imag * -1 + 1j * S.real).astype(np.complex64))}


def check_ibm_ties(make_engine, strict=True):
    """-> {tie: {mask: fraction of the planted ties answered 1}}; strict: every one must be 1, as the reference answers."""
    eng = _small_engine(make_engine)
    out = {}
    for what, (S, N) in tie_inputs().items():
        assert np.array_equal(np.abs(S), np.abs(N)), what
        for kind in ('ibm1', 'ibm2'):
            assert ref_mask32(S, N, kind).all(), (what, kind, 'the reference answers 1 on a tie')
            m = eng.tf_mask(S, N, type=kind, bin_thr=0.0).numpy()
            out.setdefault(what, {})[kind] = float(np.mean(m == 1))
            if strict:
                assert np.all(m == 1), f'{what} {kind}: {int((m != 1).sum())} of {m.size} exact ties answered 0'
    return out


GEOMETRY = (1, 255, 256, 257, 8192 * 256 + 257, 16384 * 256 + 257)         # the grid holds 16384 blocks of 256: the last enters the stride loop


def check_geometry(make_engine, sizes=GEOMETRY):
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(15)
    worst = 0.0
    for n in sizes:
        S, N = _gauss(rng, n), _gauss(rng, n)
        worst = max(worst, compare_mask(eng.tf_mask(S, N, type='irm1').numpy(), S, N, 'irm1', 0.0, f'n = {n}'))
    return worst


def check_mask_batch_independence(make_engine, parts=(1, 255, 257, 700)):
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(16)
    S, N = [_gauss(rng, n) for n in parts], [_gauss(rng, n) for n in parts]
    for kind in ('irm1', 'iam2', 'ibm1'):
        whole = eng.tf_mask(np.concatenate(S), np.concatenate(N), type=kind).numpy()
        _same_bits(whole, np.concatenate([eng.tf_mask(s, n, type=kind).numpy() for s, n in zip(S, N)]), f'concatenation, {kind}')


# ---- B. per-channel masks of the path --------------------------------------------------------------------------------------------------
def channel_cases(mics=(1, 2, 3, 8)):
    return [(M, ref, kind) for M in mics for ref in sorted({0, M - 1}) for kind in ('irm1', 'iam2', 'ibm1')]


def _scene(M, R=2, K=2, L=1536, seed=17):
    rng = np.random.default_rng(seed + M)
    s = (0.3 * rng.standard_normal((R, K, M, L))).astype(np.float32)
    n = rng.standard_normal((R, K, M, L)).astype(np.float32)
    s[1, :, :, :600] = 0
    return s, n


def check_channel_masks(make_engine, M, ref_mic, kind):
    s, n = _scene(M)
    R, K, _, L = s.shape
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, mask=kind, ref_mic=ref_mic)
    got = eng.tango_reference(s + n, s, n, steps=3, want=('masks_z', 'mask_w'))
    Xs = eng.stft(s.reshape(R * K, M, L)).numpy()
    Xn = eng.stft(n.reshape(R * K, M, L)).numpy()
    for name, ch in (('masks_z', ref_mic), ('mask_w', 0)):
        want = eng.tf_mask(np.ascontiguousarray(Xs[..., ch]), np.ascontiguousarray(Xn[..., ch]), type=kind).numpy()
        _same_bits(got[name].numpy().reshape(want.shape), want, f'{name}, M = {M}, ref_mic = {ref_mic}, {kind}')


def check_compressed_masks(make_engine, M=2, kinds=('irm1', 'iam2', 'ibm1')):
    """mask_for_z = 'compressed': the k_tf_mask launch on (z_s, z_n) inside the call makes the mask that splits the EXCHANGED rows; it
    stays in the workspace and is seen only through yf (tests/parity_checks.py holds that against the oracle).  The returned masks_z is
    still the step-1 mask at the reference microphone: held here bit for bit, NaN positions included, with the compressed signals
    finite."""
    s, n = _scene(M)
    R, K, _, L = s.shape
    for kind in kinds:
        eng = make_engine(rooms=R, nodes=K, mics=M, length=L, mask=kind, ref_mic=M - 1)
        got = eng.tango_reference(s + n, s, n, mask_for_z='compressed', steps=3, want=('masks_z', 'z_s', 'z_n', 'yf'))
        Xs, Xn = eng.stft(s.reshape(R * K, M, L)).numpy(), eng.stft(n.reshape(R * K, M, L)).numpy()
        want = eng.tf_mask(np.ascontiguousarray(Xs[..., M - 1]), np.ascontiguousarray(Xn[..., M - 1]), type=kind).numpy()
        _same_bits(got['masks_z'].numpy().reshape(want.shape), want, f'masks_z with compressed rows, {kind}')
        finite = np.isfinite(want).reshape(R, K, -1).all(-1)             # 'iam' is NaN in the frames where both images are silent
        for nm in ('z_s', 'z_n', 'yf'):
            assert np.isfinite(got[nm].numpy()[finite]).all(), (nm, kind)


# ---- C. oracle masks from time signals ---------------------------------------------------------------------------------------------
ORACLE_VALUE_KINDS = ('irm1', 'irm2', 'iam1', 'iam2')
ORACLE_KINDS = ORACLE_VALUE_KINDS + ('ibm1', 'ibm2')


def oracle_cases(cut=False):
    """(n_fft, pad, T, L, n_sig): a short run of frames, a full run (16), a run plus one, two runs plus one, a second block (65 frames: five
    runs, four waves per block); wave-item counts that are no multiple of 4; L = (T - 1) hop + a remainder, once with none."""
    rng = np.random.default_rng(18)
    cases = []
    for n_fft in (512, 1024):
        hop = n_fft // 2
        for pad in ('reflect', 'constant'):
            for i, T in enumerate((15, 16, 17, 33, 65)):
                cases.append((n_fft, pad, T, (T - 1) * hop + int(rng.integers(1, hop)), (3, 1, 5)[(i + (pad == 'constant')) % 3]))
            cases.append((n_fft, pad, 16, 15 * hop, 5 if pad == 'reflect' else 3))
    if cut:
        keep = {(512, 'reflect', 17), (512, 'constant', 65), (1024, 'constant', 15), (1024, 'reflect', 33)}
        cases = [c for c in cases if c[:3] in keep and c[3] % (c[0] // 2)]
    return cases


def _frames(x, n_fft, pad, dtype):
    """The windowed frames stft_oracle.stft transforms, (n_sig, T, n_fft), in `dtype`."""
    half, hop = n_fft // 2, n_fft // 2
    xp = np.pad(np.asarray(x, dtype), [(0, 0), (half, half)], mode=pad)
    T = 1 + x.shape[-1] // hop
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    return xp[:, idx] * so.hann_periodic(n_fft).astype(dtype)


def _sens(aS, aN, aY, kind, d=0.0):
    """G: first-order sensitivity of the mask to each magnitude, no division by |S|; for 'ibm' that of xi.  d > 0: the factor
    |S|^(p - 1) is taken at |S| + d, which makes d G a bound of the change under a perturbation of SIZE d and not only its first-order term
    (mean value theorem) -- for p >= 2 the first-order term vanishes identically in a silent bin, while a spectrum of the size of the rounding
    unit there is legitimate: the kernel transforms s and n as one complex signal, so the rounding of n's transform leaks into S.
    For p = 1 the two are the same formula."""
    p = int(kind[3])
    with np.errstate(all='ignore'):
        if kind.startswith('iam'):
            return p * ((aS + d) ** (p - 1) / aY ** p + 2 * (aS / aY) ** p / aY)
        an = np.maximum(aN, EPS)
        xi = (aS / an) ** p
        g = p * ((aS + d) ** (p - 1) / an ** p + xi / an)
        return g if kind.startswith('ibm') else g / (1 + xi) ** 2


def _worst_ratio(err, ref, dG):
    """max (err - 4 2^-24 |ref|)+ / (delta G): the part of the error that the bar's first term has to cover (the second term is the rounding of
    the mask value itself: a mask within 1e-7 of 1 is half an ulp off whatever the spectra are).  A bin whose sensitivity is exactly 0 (a
    silent bin of a p >= 2 mask) must have no error at all."""
    err = np.maximum(err - 4 * U * np.abs(ref), 0)
    assert not np.any((dG == 0) & (err != 0))
    return float(np.max(err / np.where(dG == 0, 1, dG), initial=0.0))


@functools.lru_cache(maxsize=None)
def oracle_case(n_fft, pad, T, L, n_sig):
    """Signals and everything on the reference side of one case, computed once; the first third of signal 0's s is exactly zero."""
    rng = np.random.default_rng(1000 * n_fft + 10 * T + n_sig + (pad == 'reflect'))
    s = (0.1 * rng.standard_normal((n_sig, L))).astype(np.float32)
    n = rng.standard_normal((n_sig, L)).astype(np.float32)
    s[0, :L // 3] = 0
    assert 1 + L // (n_fft // 2) == T
    S = np.swapaxes(so.stft(s, n_fft, n_fft // 2, pad, np.complex128), -1, -2)            # (n_sig, T, F)
    N = np.swapaxes(so.stft(n, n_fft, n_fft // 2, pad, np.complex128), -1, -2)
    fs, fn = _frames(s, n_fft, pad, np.float64), _frames(n, n_fft, pad, np.float64)
    delta = (U * np.sqrt(n_fft) * (np.linalg.norm(fs, axis=-1) + np.linalg.norm(fn, axis=-1)))[..., None]
    S32 = scipy.fft.rfft(_frames(s, n_fft, pad, np.float32), axis=-1)
    N32 = scipy.fft.rfft(_frames(n, n_fft, pad, np.float32), axis=-1)
    assert S32.dtype == np.complex64
    out = {'s': s, 'n': n, 'delta': delta, 'kinds': {}}
    aS, aN, aY = np.abs(S), np.abs(N), np.abs(S + N)
    for kind in ORACLE_KINDS:
        with np.errstate(all='ignore'):
            ref = np.asarray(mo.tf_mask(S, N, kind), np.float64)
            f32 = np.asarray(mo.tf_mask(S32, N32, kind), np.float64)
        G = _sens(aS, aN, aY, kind, (4 if kind.startswith('ibm') else C_ORACLE) * delta)
        rec = {'ref': ref, 'G': G}
        if kind.startswith('ibm'):
            xi = (aS / np.maximum(aN, EPS)) ** int(kind[3])
            rec['clear'] = np.abs(xi - 1.0) > 4 * delta * G
        else:
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(f32), ~fin), 'the float32 restatement is NaN where the oracle is, and nowhere else'
            rec['f32_ratio'] = _worst_ratio(np.abs(f32[fin] - ref[fin]), ref[fin], (delta * G)[fin])
        out['kinds'][kind] = rec
    return out


def f32_restatement_ratio(cases=None):
    """The worst err / (delta G) of the float32 restatement over the value kinds of every case: C_ORACLE is 4 x this."""
    return max(oracle_case(*c)['kinds'][k]['f32_ratio'] for c in (cases or oracle_cases()) for k in ORACLE_VALUE_KINDS)


def ibm_band_fraction(cases=None):
    return max(float(1 - oracle_case(*c)['kinds'][k]['clear'].mean()) for c in (cases or oracle_cases()) for k in ('ibm1', 'ibm2'))


def check_oracle_case(make_engine, case, kinds=ORACLE_KINDS):
    """Every bin of every frame.  -> the kernel's worst err / (delta G) over the value kinds (the restatement's quantity)."""
    n_fft, pad, T, L, n_sig = case
    ref = oracle_case(*case)
    worst = 0.0
    for kind in kinds:
        eng = make_engine(rooms=n_sig, nodes=1, mics=1, length=L, n_fft=n_fft, mask=kind, pad_mode=pad)
        assert (eng.T, eng.F) == (T, n_fft // 2 + 1)
        m = eng.mask_oracle(ref['s'], ref['n']).numpy().astype(np.float64)
        rec = ref['kinds'][kind]
        if kind.startswith('ibm'):
            bad = rec['clear'] & (m != rec['ref'])
            assert not bad.any(), f'{case} {kind}: {int(bad.sum())} wrong decisions outside the band, first at {np.argwhere(bad)[0]}'
            assert np.all((m == 0) | (m == 1))
            continue
        fin = np.isfinite(rec['ref'])
        assert np.array_equal(np.isnan(m), ~fin), f'{case} {kind}: NaN where the oracle is NaN ({int((~fin).sum())} bins) and nowhere else'
        err = np.where(fin, np.abs(m - np.where(fin, rec['ref'], 0)), 0)
        dG = np.where(fin, ref['delta'] * rec['G'], 1)
        bar = C_ORACLE * dG + 4 * U * np.abs(np.where(fin, rec['ref'], 0))
        bad = err > bar
        assert not bad.any(), f'{case} {kind}: {int(bad.sum())} of {bad.size} bins beyond the bar, worst err / bar {float((err / bar)[bad].max()):.3g}, first at {np.argwhere(bad)[0]}'
        for f, name in ((0, 'DC'), (-1, 'Nyquist')):                     # the Nyquist bin is stored by lane 0 alone
            assert np.all(err[..., f] <= bar[..., f]), (case, kind, name)
        worst = max(worst, _worst_ratio(err[fin], rec['ref'][fin], dG[fin]))
    return worst


# ---- D. VAD mask ----------------------------------------------------------------------------------------------------------------
VAD_FAMILIES = ('bursts', 'bursts + DC', 'quantised 1/32768', 'half zeroed', 'quantised 1/8', 'zeros')


def vad_signals(L, rng):
    """(6, L) float32: one signal of every family.  (A constant non-zero signal is not a test input, see the module docstring.)"""
    def bursts(level):
        gate = np.zeros(L)
        i = 0
        while i < L:
            n_on, n_off = int(rng.integers(1, max(2, L // 3))), int(rng.integers(1, max(2, L // 3)))
            gate[i:i + n_on] = 1
            i += n_on + n_off
        return level * rng.standard_normal(L) * gate
    lv = lambda: 10.0 ** rng.uniform(-4, 0)
    x = np.zeros((6, L))
    x[0] = bursts(lv())
    x[1] = bursts(lv()) + rng.uniform(-1, 1)
    x[2] = np.round(bursts(lv()) * 32768) / 32768
    x[3] = bursts(lv()) * (rng.random(L) < 0.5)
    x[4] = np.round(bursts(1.0) * 8) / 8
    return x.astype(np.float32)


def vad_lengths(n_fft, cut=False):
    hop = n_fft // 2
    if cut:
        return (300, 512, 513, 1279, 2501) if n_fft == 512 else (700, 1025, 2501)
    return (hop + 1, 300 if n_fft == 512 else 700, n_fft - 1, n_fft, n_fft + 1, 3 * n_fft - 1, 3 * n_fft, 5 * hop - 1, 5 * hop + 1, 2501, 12801, 5000, 7001)


def vad_reference(x, n_fft):
    F, T = n_fft // 2 + 1, 1 + x.shape[-1] // (n_fft // 2)
    return np.stack([mo.ivad_mask(xi, (F, T), n_fft, n_fft // 2).T for xi in x])               # (n_sig, T, F)


def check_vad(make_engine, n_fft, L, seed=0, alone=(0, 3)):
    """Zero frames wrong, constant over frequency; the signals in `alone` also run alone, bit for bit.  -> frames compared."""
    x = vad_signals(L, np.random.default_rng(19 + seed + L))
    eng = make_engine(rooms=len(x), nodes=1, mics=1, length=L, n_fft=n_fft, lazy_scratch=True,
                      pad_mode='reflect' if L > n_fft // 2 else 'constant')
    m = eng.mask_ivad(x).numpy()
    assert np.all(m == m[:, :, :1]), f'L = {L}: the mask varies over frequency'
    ref = vad_reference(x, n_fft)
    bad = m[:, :, 0] != ref[:, :, 0]
    assert not bad.any(), f'n_fft {n_fft}, L = {L}: {int(bad.sum())} frames wrong, (family, frame): {[(VAD_FAMILIES[i], int(t)) for i, t in np.argwhere(bad)[:6]]}'
    for i in alone:
        _same_bits(eng.mask_ivad(x[i:i + 1]).numpy()[0], m[i], f'L = {L}: signal {i} alone')
    return int(bad.size)


def check_vad_refusal(make_engine, n_fft=512):
    hop = n_fft // 2
    eng = make_engine(rooms=1, nodes=1, mics=1, length=4096 * hop + 1, n_fft=n_fft, lazy_scratch=True)
    _raises(lambda: eng.mask_ivad(np.zeros((1, 4096 * hop + 1), np.float32)), 'disco_mask_ivad: signal longer than 4096 hops')
    rng = np.random.default_rng(20)
    S, N = _gauss(rng, 300), _gauss(rng, 300)
    compare_mask(eng.tf_mask(S, N, type='irm1').numpy(), S, N, 'irm1', 0.0, 'after the refusal')


def vad_restatement(x, n_fft):
    """NumPy restatement of k_vad_mask's arithmetic for one float32 signal -> the frame decisions (len = ceil(L / hop)): float64 mean
    rounded to float32, float32 squares, the two order statistics around (L - 1) q with q = float32(0.99), a float32 threshold."""
    x = np.asarray(x, np.float32)
    L, hop = x.size, n_fft // 2
    mean = np.float32(np.sum(x.astype(np.float64)) / L)
    d = x - mean
    x2 = np.abs(d * d)
    assert x2.dtype == np.float32
    vidx = (L - 1) * float(np.float32(0.99))
    k = int(vidx)
    srt = np.sort(x2)
    v_lo, v_hi = float(srt[k]), float(srt[min(k + 1, L - 1)])
    thr = np.float32(0.001) * np.float32(v_lo + (v_hi - v_lo) * (vidx - k))
    over = x2 > thr
    vad = np.zeros(L)
    for w in range(int(np.ceil((L - n_fft) / hop + 1))):
        lo, hi = w * hop, min(w * hop + n_fft, L)
        if over[lo:hi].sum() >= (hi - lo) // 2:
            vad[lo:hi] = 1
    return vad[::hop]


# ---- E. level statistics ------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = ((3, 1, 0, 1), (2, 255, 0, 255), (2, 256, 0, 256), (2, 257, 1, 257), (5, 1000, 999, 1000), (2, 1000, 500, 500), (4, 5000, 16, 4999))


def check_pair_stats(make_engine):
    eng = _small_engine(make_engine)
    rng = np.random.default_rng(21)
    worst = 0.0
    for j, (n_sig, L, start, stop) in enumerate(PAIR_SHAPES):
        a = rng.standard_normal((n_sig, L)).astype(np.float32)
        b = rng.standard_normal((n_sig, L)).astype(np.float32)
        a[:, ::3] = 0
        b[:, ::5] = 0
        aliased = j == 3
        if aliased:
            b = a
        xa, xb = a[:, start:stop].astype(np.float64), b[:, start:stop].astype(np.float64)
        a[:, :start] = np.nan
        a[:, stop:] = np.nan
        b[:, :start] = np.nan
        b[:, stop:] = np.nan
        st = eng.pair_stats(a, a if aliased else b, start, stop).numpy()
        assert np.array_equal(st[:, 0], (xa != 0).sum(1)) and np.array_equal(st[:, 3], (xb != 0).sum(1)) and np.all(st[:, 7] == stop - start), (n_sig, L, start, stop)
        for col, terms in ((1, xa), (2, xa * xa), (4, xb), (5, xb * xb), (6, xa * xb)):
            tol = 8 * 2.0 ** -53 * np.abs(terms).sum(1)
            err = np.abs(st[:, col] - np.array([np.sum(t) for t in terms]).reshape(n_sig))
            assert np.all(err <= tol), ((n_sig, L, start, stop), col, err, tol)
            worst = max(worst, float(err.max()))
    return worst


def butter_bank(n_bands, fs=16000.0):
    fc = np.geomspace(150.0, 6000.0, n_bands) if n_bands > 1 else np.array([150.0])
    b, a = np.zeros((n_bands, 9)), np.zeros((n_bands, 9))
    for i, f in enumerate(fc):
        b[i], a[i] = scipy.signal.butter(4, np.array([f * 2 ** (-1 / 6), f * 2 ** (1 / 6)]) * 2 / fs, btype='bandpass', output='ba')
    return b, a, fc


def band_bank(name):
    """'third16k' | 'third8k' (the banks of fw_snr) | a number of Butterworth bands -> b, a (n_bands, 9), centre frequencies (n_bands,)."""
    if isinstance(name, str):
        fs = {'third16k': 16000, 'third8k': 8000}[name]
        F = meo.band_importance(fs)[0]
        return meo.third_octave_filterbank(F, fs, order=4) + (np.asarray(F, float),)
    return butter_bank(name)


def _pooled(d, fc):
    """d (n_bands,) -> per band, the worst d over the bands whose centre lies inside its own pass band (within a sixth of an octave).
    The conditioning of the 'ba' form is a smooth function of the centre frequency, and the worst of three signals (one signal per
    workgroup: n_bands > 128) is a noisy estimate of it; in the dense banks the neighbours a few percent away are further draws of
    the same quantity.  In the third-octave banks a band has no such neighbour and keeps its own figure."""
    near = np.abs(np.log2(fc[:, None] / fc[None, :])) <= 1 / 6 + 1e-9
    return np.where(near, d[None, :], 0).max(1)


BANKS = ('third16k', 'third8k', 1, 7, 8, 9, 100, 129, 256)
SPANS = ((700, 0, 700), (700, 3, 515), (300, 40, 41), (256, 0, 256), (257, 0, 257), (600, 100, 100))


def spb_of(n_bands):
    return min(32, 256 // n_bands)


def lfilter_ld(b, a, x):
    """scipy.signal.lfilter's recurrence (direct form II transposed, zero initial state) in long double: b, a (n_bands, 9), x (n_sig, n)
    -> (n_sig, n_bands, n)."""
    ld = np.longdouble
    b, a = b.astype(ld) / a[:, :1].astype(ld), a.astype(ld) / a[:, :1].astype(ld)
    x = x.astype(ld)
    z = np.zeros((x.shape[0], b.shape[0], 9), ld)
    y = np.zeros((x.shape[0], b.shape[0], x.shape[1]), ld)
    for i in range(x.shape[1]):
        xv = x[:, None, i, None]
        yi = b[None, :, :1] * xv + z[:, :, :1]
        z[:, :, :8] = b[None, :, 1:] * xv + z[:, :, 1:] - a[None, :, 1:] * yi
        y[:, :, i] = yi[:, :, 0]
    return y


def _band_sums(y, gate):
    """y (n_sig, n_bands, n), gate (n_sig, n) 0/1 or None -> sum y, sum y^2, sum |y| over the scored samples, each (n_sig, n_bands)."""
    g = 1 if gate is None else gate[:, None, :].astype(y.dtype)
    return (y * g).sum(-1), (y * y * g).sum(-1), (np.abs(y) * g).sum(-1)


@functools.lru_cache(maxsize=None)
def band_case(bank, span):
    """Signals (2 spb + 1 of them), gate and the reference side of one (bank, span): long-double sums and SciPy's distance from them."""
    b, a, fc = band_bank(bank)
    L, start, stop = span
    n_sig = 2 * spb_of(b.shape[0]) + 1
    rng = np.random.default_rng(22 + 7 * L + start + 1000 * b.shape[0])
    x = rng.standard_normal((n_sig, L)).astype(np.float32)
    x[:, :L // 5] = 0
    gate = (rng.random((n_sig, L)) < 0.6).astype(np.float32)
    xs, gs = x[:, start:stop], gate[:, start:stop]
    yl = lfilter_ld(b, a, xs)
    ysp = np.stack([scipy.signal.lfilter(b[i], a[i], xs.astype(np.float64), axis=-1) for i in range(b.shape[0])], axis=1) if stop > start else np.zeros(yl.shape)
    x_nan, g_nan = x.copy(), gate.copy()
    for v in (x_nan, g_nan):
        v[:, :start] = np.nan
        v[:, stop:] = np.nan
    out = {'b': b, 'a': a, 'x': x_nan, 'gate': g_nan}
    lead = np.minimum(np.maximum(L // 5 - start, 0), stop - start)                  # exact zeros at the head of the span
    for mode, g in (('ungated', None), ('gated', gs)):
        s1, s2, sabs = _band_sums(yl, g)
        _, p2, _ = _band_sums(ysp.astype(np.longdouble), g)
        _, _, l1 = _band_sums(ysp.astype(np.longdouble) - yl, g)               # sum |y_scipy - y|: see the module docstring on sum y
        with np.errstate(all='ignore'):
            d1 = np.where(sabs > 0, l1 / np.where(sabs > 0, sabs, 1), 0).astype(np.float64)
            d2 = np.where(s2 > 0, np.abs(p2 - s2) / np.where(s2 > 0, s2, 1), 0).astype(np.float64)
        cnt = np.full((n_sig, b.shape[0]), float(stop - start - lead)) if g is None else np.repeat(g.sum(-1, dtype=np.float64)[:, None], b.shape[0], 1)
        out[mode] = {'cnt': cnt, 's1': s1, 's2': s2, 'sabs': sabs, 'scipy1': _pooled(d1.max(0), fc), 'scipy2': _pooled(d2.max(0), fc)}
    return out


def check_band_case(make_engine, bank, span, n_sigs=None):
    """-> per mode, the worst over the bands of (kernel distance / SciPy's distance) for sum y^2, and both distances of the lowest band."""
    ref = band_case(bank, span)
    eng = _small_engine(make_engine)
    L, start, stop = span
    spb = spb_of(ref['b'].shape[0])
    out = {}
    for mode in ('ungated', 'gated'):
        r = ref[mode]
        full = None
        for n_sig in sorted(set(n_sigs or (1, spb, spb + 1, 2 * spb + 1)), reverse=True):
            st = eng.band_stats(ref['x'][:n_sig], ref['b'], ref['a'], start, stop, gate=ref['gate'][:n_sig] if mode == 'gated' else None).numpy()
            what = f'bank {bank}, span {span}, {mode}, n_sig {n_sig}'
            assert np.array_equal(st[..., 0], r['cnt'][:n_sig]), (what, 'counts')
            with np.errstate(all='ignore'):
                d1 = np.abs(st[..., 1] - r['s1'][:n_sig]).astype(np.float64)
                d2 = np.abs(st[..., 2] - r['s2'][:n_sig]).astype(np.float64)
                bar1 = np.maximum(BAND_FACTOR * r['scipy1'], BAND_FLOOR)[None, :] * r['sabs'][:n_sig].astype(np.float64)
                bar2 = np.maximum(BAND_FACTOR * r['scipy2'], BAND_FLOOR)[None, :] * r['s2'][:n_sig].astype(np.float64)
            assert np.all(d1 <= bar1), (what, 'sum y', np.argwhere(d1 > bar1)[:4], float((d1 / np.where(bar1 > 0, bar1, 1)).max()))
            assert np.all(d2 <= bar2), (what, 'sum y^2', np.argwhere(d2 > bar2)[:4], float((d2 / np.where(bar2 > 0, bar2, 1)).max()))
            if full is None:
                full = st
                s2 = r['s2'].astype(np.float64)
                rel = np.where(s2 > 0, d2 / np.where(s2 > 0, s2, 1), 0).max(0)
                out[mode] = {'kernel_over_scipy_worst_band': float((rel / np.maximum(r['scipy2'], BAND_FLOOR / BAND_FACTOR)).max()),
                             'kernel_lowest_band': float(rel[0]), 'scipy_lowest_band': float(r['scipy2'][0])}
            else:                                                           # a shorter batch: the same rows, bit for bit
                _same_bits(st, full[:n_sig], what + ' against the rows of the longest batch')
    return out


def check_band_rows_alone(make_engine, bank='third16k', span=(700, 3, 515)):
    """Rows of a batch of 2 spb + 1 signals (both sides of both workgroup boundaries) against the same signal run alone, bit for bit."""
    ref = band_case(bank, span)
    eng = _small_engine(make_engine)
    _, start, stop = span
    spb = spb_of(ref['b'].shape[0])
    for gated in (False, True):
        run = lambda x, g: eng.band_stats(x, ref['b'], ref['a'], start, stop, gate=g if gated else None).numpy()
        full = run(ref['x'], ref['gate'])
        for i in (0, spb - 1, spb, 2 * spb - 1, 2 * spb):
            _same_bits(run(ref['x'][i:i + 1], ref['gate'][i:i + 1])[0], full[i], f'bank {bank}, row {i} alone, gated {gated}')


def check_metrics_batch(fs=16000, L=2000, start=100):
    """disco_amd.metrics on a batch of 2 spb + 1 signals (one of them all zero): the per-signal calls bit for bit, oracle/metrics_oracle.py
    at 2e-4 dB, NaN for the all-zero signal alone.  Uses the package's own engine (the emulated tier binds it to the emulator)."""
    from disco_amd import metrics as dm
    n_sig = 2 * spb_of(len(meo.band_importance(fs)[0])) + 1
    zero = n_sig // 2
    rng = np.random.default_rng(23)
    s = (0.5 * rng.standard_normal((n_sig, L))).astype(np.float32)
    n = (0.2 * rng.standard_normal((n_sig, L))).astype(np.float32)
    so_ = (s + 0.1 * rng.standard_normal((n_sig, L))).astype(np.float32)
    for v in (s, n, so_):
        v[:, :300] = 0
        v[zero] = 0
    vt = (rng.random((n_sig, L)) < 0.7).astype(np.float32)
    vn = (rng.random((n_sig, L)) < 0.5).astype(np.float32)
    vt[zero] = 0
    sl = slice(start, L)
    calls = {
        'snr': (lambda i: dm.snr(s[i], n[i], start=start), lambda i: meo.snr(s[i, sl], n[i, sl])),
        'sd': (lambda i: dm.sd(so_[i], s[i], start=start), lambda i: meo.sd(so_[i, sl], s[i, sl])),
        'si_sdr': (lambda i: dm.si_sdr(s[i], so_[i], start=start), lambda i: meo.si_sdr(s[i, sl], so_[i, sl])),
        'fw_snr': (lambda i: dm.fw_snr(s[i], n[i], fs, start=start)[1], lambda i: meo.fw_snr(s[i, sl], n[i, sl], fs)[1]),
        'fw_snr_vad': (lambda i: dm.fw_snr(s[i], n[i], fs, vad_tar=vt[i], vad_noi=vn[i], start=start)[1],
                       lambda i: meo.fw_snr(s[i, sl], n[i, sl], fs, vt[i, sl], vn[i, sl])[1]),
        'fw_sd': (lambda i: dm.fw_sd(so_[i], s[i], fs, start=start)[1], lambda i: meo.fw_sd(so_[i, sl], s[i, sl], fs)[1]),
    }
    worst = {}
    rows = np.arange(n_sig)
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for name, (mine, oracle) in calls.items():
                batch = np.asarray(mine(slice(None)), np.float64)
                assert batch.shape == (n_sig,), (name, batch.shape)
                single = np.array([np.asarray(mine(slice(i, i + 1)), np.float64).reshape(()) for i in rows])
                _same_bits(batch, single, f'{name}: the batch against the per-signal calls')
                assert np.isnan(batch[zero]) and np.isfinite(np.delete(batch, zero)).all(), (name, 'NaN for the all-zero signal and for no other')
                ref = np.array([float(oracle(i)) for i in rows])
                assert np.isnan(ref[zero]), name
                worst[name] = float(np.abs(np.delete(batch - ref, zero)).max())
                assert worst[name] < 2e-4, (name, worst[name])
    return worst
