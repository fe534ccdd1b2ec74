"""Checks of the meeting-room generator: the leave-one-out mixes (csrc/k_roomsynth.h k_source_mix), the per-source masks and the mix spectrum in
one transform pass (csrc/k_stft.h k_source_masks<512 | 1024, 1..4 pairs>), and the Python surface built on them
(disco_amd.dataset_utils.simulate_meetings / sir_at_nodes / sir_valid / get_value_range / meeting_rooms / meeting_masks).

Shared by tests/test_gpu_meeting.py (real MI355X, `-m gpu`), tests/test_meeting_emulated.py (the same kernel sources under the hipemu CPU
emulator, the smallest cases) and tests/test_meeting_cpu.py (the reference side alone: the constant behind the mask bar, the share of
undecided 'ibm' bins, the fixture of the acceptance rule).  `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library
under test; the checks of the package-level functions use the package's own engine (the emulated tier binds it to the emulator).

References and bars, none taken from a kernel's output:
  mixes     NumPy float32 sums in the stated order -- y = ((img_0 + img_1) + img_2) + ..., n = the images j != target added in ascending j --
            compared bit for bit (NaN where NumPy has NaN, the same bits everywhere else).
  masks     the reference's own order of operations in float64: oracle.stft_oracle.stft of the float64 TIME-DOMAIN sums (source i, the sum
            of the others, the sum of all), then oracle.mwf_oracle.tf_mask.  Bar of a bin, the one of mask_metric_checks.check_oracle_case
            generalised: err <= C_MEETING delta G + 4 2^-24 |ref|, delta = 2^-24 sqrt(n_fft) sum_j |windowed frame of source j|_2 over ALL S
            sources (every transform's rounding leaks into every N_i, and through the shared complex FFT into its partner), G =
            mask_metric_checks._sens.  C_MEETING is 4 x the worst (err - 4 2^-24 |ref|)+ / (delta G) of the float32 NumPy restatement
            (scipy.fft.rfft of the float32 frames of every source, complex64 sums of the spectra in ascending order, the mask in float32)
            over `mask_cases()`; tests/test_meeting_cpu.py recomputes it and holds the constant below to it.  NaN / inf exactly where
            the float64 reference has them.  The mix spectrum: |mix - ref| <= C_MEETING delta per bin.
  'ibm'     decisions exact outside the band |xi - 1| <= 4 delta G.  A bin whose float64 noise magnitude is exactly zero (S = 2, the other
            source silent over the whole frame) is never excluded: it is held to the float32 restatement's decision.  The band holds at
            most 0.1 % of a case's bins (asserted on the reference side by the CPU tier).
  lengths, batches    bit equality of a room in a batch with the room run alone.
  SIRs      metrics.bss_eval_sources called by hand on NumPy sums, bit for bit; the float64 Gram oracle of tests/bss_checks.py at its TOL_DB.
  rule      sir_valid / get_value_range against tests/golden/meeting_ref.npz, the reference's own functions run by
            tests/golden/make_golden_meeting.py.
  rooms     simulate_meetings equals the same public calls made by hand from the returned RIRs on (Engine.ism_rir sums with float atomics,
            so the RIRs themselves are held to the float64 oracle at the 5e-6 of parity_checks.check_ism_rir, as check_simulate_rooms does).
"""
import functools
import os

import numpy as np
import scipy.fft

import mask_metric_checks as mc
from oracle import mwf_oracle as mo
from oracle import stft_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = mc.U
C_MEETING = 0.469             # 4 x the float32 restatement's worst err / (delta G) over mask_cases() (tests/test_meeting_cpu.py recomputes it)
MASK_KINDS = ('irm1', 'irm2', 'iam1', 'ibm1')
VALUE_KINDS = ('irm1', 'irm2', 'iam1')
MIX_SOURCES = (2, 3, 4, 8)
MIX_LENGTHS = (1, 1023, 1024, 1025, 4099)        # odd lengths take the scalar route; 1024 is MIX_CHUNK


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b, what):
    """The same bits, except that any NaN answers any NaN (np.array_equal(..., equal_nan=True), with -0 told from +0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == 'c':
        a, b = a.view(a.real.dtype), b.view(b.real.dtype)
    bad = (_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}'


def _small_engine(make_engine):
    return make_engine(rooms=1, nodes=1, mics=1, length=1024)


def _refused(fn, text, exc=ValueError):
    try:
        fn()
    except exc as e:
        assert text in str(e), (text, str(e))
    else:
        raise AssertionError(f'not refused: {text}')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, 'meeting_ref.npz')))


def levelled(shape, seed):
    """Gaussian sources (S, ...) float32 whose levels are spread over 1.5 decades, in an order drawn with the seed."""
    rng = np.random.default_rng(seed)
    S = shape[0]
    level = 10.0 ** rng.permutation(np.linspace(-1.5, 0.0, S))
    return (level.reshape((S,) + (1,) * (len(shape) - 1)) * rng.standard_normal(shape)).astype(np.float32)


# ---- leave-one-out mixes -----------------------------------------------------------------------------------------------------------------
def mix_reference(img, target, stop=None):
    """disco_source_mix in NumPy float32: img (S, R, n_mic, L), target (n_mic,), stop None or broadcast over (R, n_mic) -> y, s, n.
    Every sum is a chain of float32 additions in the stated order; at and beyond a stop exact zeros, whatever the inputs hold there."""
    img = np.asarray(img, np.float32)
    S, R, n_mic, L = img.shape
    with np.errstate(invalid='ignore'):
        y = img[0].copy()
        for j in range(1, S):
            y = y + img[j]
        s, n = np.empty_like(y), np.empty_like(y)
        for c in range(n_mic):
            s[:, c] = img[target[c], :, c]
            others = [j for j in range(S) if j != target[c]]
            acc = img[others[0], :, c].copy()
            for j in others[1:]:
                acc = acc + img[j, :, c]
            n[:, c] = acc
    assert y.dtype == np.float32 and n.dtype == np.float32
    if stop is not None:
        beyond = np.arange(L)[None, None, :] >= np.broadcast_to(np.asarray(stop), (R, n_mic))[:, :, None]
        y, s, n = (np.where(beyond, np.float32(0), a) for a in (y, s, n))
    return y, s, n


def mix_scene(S, L, seed, R=3, n_mic=5):
    rng = np.random.default_rng(seed)
    img = levelled((S, R, n_mic, L), seed)
    target = rng.integers(0, S, n_mic)
    target[:2] = (0, S - 1)                                                  # the first and the last source are somebody's target
    return img, target.astype(np.int32)


def check_source_mix_bits(make_engine, sources=MIX_SOURCES, lengths=MIX_LENGTHS):
    """Every S x L: without stops; with the stops 0, 1, L - 1 and L, one per room, and NaN planted at and beyond every stop."""
    eng = _small_engine(make_engine)
    for S in sources:
        for L in lengths:
            img, target = mix_scene(S, L, 100 * S + L % 97)
            what = f'S {S}, L {L}'
            for name, got, ref in zip('ysn', eng.source_mix(img, target), mix_reference(img, target)):
                _same_bits(got, ref, f'{what}: {name}')
            for stops in ((0, 1, max(L - 1, 0)), (L, max(L - 1, 0), min(1, L))):
                stop = np.array(stops)[:, None]
                dirty = img.copy()
                for r, st in enumerate(stops):
                    dirty[:, r, :, st:] = np.nan
                for name, got, ref in zip('ysn', eng.source_mix(dirty, target, stop=stop), mix_reference(img, target, stop)):
                    assert not np.isnan(got).any(), f'{what}, stops {stops}: a NaN beyond a stop reached {name}'
                    _same_bits(got, ref, f'{what}, stops {stops}: {name}')


def check_source_mix_each_output_alone(make_engine, cases=((3, 1024), (4, 1025), (8, 4099))):
    """Each output alone (the others not wanted) equals the full call; a per-channel stop; rows one float off 16-byte alignment."""
    eng = _small_engine(make_engine)
    for S, L in cases:
        img, target = mix_scene(S, L, 7 * S + L)
        stop = np.random.default_rng(L).integers(0, L + 1, (3, 5))
        full = mix_reference(img, target, stop)
        for k, name in enumerate('ysn'):
            want = [i == k for i in range(3)]
            got = eng.source_mix(img, target, stop=stop, want_y=want[0], want_s=want[1], want_n=want[2])
            assert all((g is None) != w for g, w in zip(got, want)), name
            _same_bits(got[k], full[k], f'S {S}, L {L}: {name} alone')
    img, target = mix_scene(3, 1024, 5)
    padded = eng.to_device(np.concatenate([np.zeros(1, np.float32), img.reshape(-1)]), np.float32)[1]
    for name, got, ref in zip('ysn', eng.source_mix(padded.part(1, img.shape), target), mix_reference(img, target)):
        _same_bits(got.numpy(), ref, f'unaligned images: {name}')


def check_source_mix_many_rows(make_engine, R=1100, n_mic=60, L=4):
    """More (row, chunk) items than the grid of 65 536 workgroups holds: the grid-stride loop."""
    eng = _small_engine(make_engine)
    img, target = mix_scene(2, L, 9, R=R, n_mic=n_mic)
    assert R * n_mic > 1 << 16
    for name, got, ref in zip('ysn', eng.source_mix(img, target), mix_reference(img, target)):
        _same_bits(got, ref, f'many rows: {name}')


def check_source_mix_nan_isolation(make_engine, S=4, L=1024):
    """A NaN in one source of one channel stays in that channel -- and, within it, out of the outputs that do not sum that source."""
    eng = _small_engine(make_engine)
    img, target = mix_scene(S, L, 11)
    for j in (int(target[1]), (int(target[1]) + 1) % S):                     # channel 1's own talker, then one of its noises
        dirty = img.copy()
        dirty[j, 2, 1, 300:310] = np.nan
        got = eng.source_mix(dirty, target)
        ref = mix_reference(dirty, target)
        clean = mix_reference(img, target)
        for name, g, r, c in zip('ysn', got, ref, clean):
            _same_bits(g, r, f'NaN in source {j}: {name}')
            touched = np.isnan(g)
            assert not touched[np.arange(3) != 2].any() and not touched[:, np.arange(5) != 1].any(), name
            _same_bits(np.where(touched, 0, g), np.where(touched, 0, c), f'NaN in source {j}: {name} elsewhere')
        assert np.isnan(got[0][2, 1, 300:310]).all()
        assert np.isnan(got[1][2, 1]).any() == (j == target[1]) and np.isnan(got[2][2, 1]).any() == (j != target[1])


def check_source_mix_refusals(make_engine):
    """S = 1, S = 9, a target outside [0, S), more than 64 channels: the code, the limit named, nothing written, the context usable."""
    from disco_amd import _lib
    from disco_amd.engine import DiscoError
    eng = _small_engine(make_engine)
    img = levelled((9, 2, 4, 64), 3)
    pi, ki = eng.to_device(img, np.float32)
    sentinel = np.full((2, 4, 64), 7.0, np.float32)
    outs = [eng.to_device(sentinel, np.float32) for _ in range(3)]
    tgt = lambda *v: np.array(v, np.int32)

    def call(S, target, n_mic=4, n_row=8, po=None):
        po = [o[0] for o in outs] if po is None else po
        return eng.lib.disco_source_mix(eng.ctx, pi, S, n_row, 64, target.ctypes.data, n_mic, None, po[0], po[1], po[2], eng.stream)
    for S, target, code, text in ((1, tgt(0, 0, 0, 0), _lib.E_UNSUPPORTED, '2 <= n_src <= 8'), (9, tgt(0, 1, 2, 8), _lib.E_UNSUPPORTED, '2 <= n_src <= 8'),
                                  (4, tgt(0, 1, 2, 4), _lib.E_ARG, 'target'), (4, tgt(0, -1, 2, 3), _lib.E_ARG, 'target')):
        assert call(S, target) == code, (S, target)
        assert text in eng.lib.disco_last_error(eng.ctx).decode(), (S, target, eng.lib.disco_last_error(eng.ctx))
    assert call(2, np.zeros(65, np.int32), n_mic=65, n_row=65) == _lib.E_UNSUPPORTED
    assert call(2, tgt(0, 1, 0, 1), n_row=7) == _lib.E_ARG
    assert call(2, tgt(0, 1, 0, 1), po=[None, None, None]) == _lib.E_ARG
    eng.sync()
    for p, k in outs:
        _same_bits(k.numpy(), sentinel, 'an output after the refusals')
    assert call(4, tgt(0, 1, 2, 3)) == 0                                     # ... and the same buffers are then taken
    ref = mix_reference(img[:4], tgt(0, 1, 2, 3))
    for (p, k), r, name in zip(outs, ref, 'ysn'):
        _same_bits(k.numpy(), r, f'after the refusals: {name}')
    _refused(lambda: eng.source_mix(img[:1], tgt(0, 0, 0, 0)), '2 <= n_src <= 8', DiscoError)
    _refused(lambda: eng.source_mix(img, tgt(0, 1, 2, 3)), '2 <= n_src <= 8', DiscoError)
    _refused(lambda: eng.source_mix(img[:3], tgt(0, 1, 2)), 'one integer per channel')
    _refused(lambda: eng.source_mix(img[:3], tgt(0, 1, 2, 0), want_y=False, want_s=False, want_n=False), 'nothing asked for')
    _refused(lambda: eng.source_mix(img[:3], tgt(0, 1, 2, 0), stop=65), 'stop')


# ---- per-source masks and the mix spectrum --------------------------------------------------------------------------------------------------
MASK_S = (2, 3, 4, 5, 8)                       # one pair, a lone last source, two pairs, a lone last source behind two pairs, four pairs
MASK_T = (2, 3, 16, 17, 33)                    # the run edges at STFT_RUN = 16
MASK_NSIG = (3, 1, 5, 3, 3)                    # with 1, 1, 1, 2, 3 runs: 3, 1, 5, 6, 9 wave items -- never a whole workgroup of 4


def mask_cases(cut=False):
    """(n_fft, pad, S, T, L, n_sig): every S and every T under each of the four (n_fft, pad) settings, S and T paired differently in each;
    L = (T - 1) hop + a remainder.  cut: the four smallest, one per setting, for the emulated tier."""
    rng = np.random.default_rng(21)
    cases = []
    for k, (n_fft, pad) in enumerate(((512, 'reflect'), (512, 'constant'), (1024, 'reflect'), (1024, 'constant'))):
        hop = n_fft // 2
        for i, S in enumerate(MASK_S):
            t = (i + k) % 5
            cases.append((n_fft, pad, S, MASK_T[t], (MASK_T[t] - 1) * hop + int(rng.integers(1, hop)), MASK_NSIG[t]))
    if cut:
        cases = [min((c for c in cases if c[:2] == key), key=lambda c: c[2] * c[3] * c[5]) for key in sorted({c[:2] for c in cases})] + \
            [c for c in cases if c[:4] == (512, 'reflect', 5, 17)]          # ... and one that crosses a run edge
    return cases


@functools.lru_cache(maxsize=None)
def mask_case(n_fft, pad, S, T, L, n_sig):
    """Images and everything on the reference side of one case, computed once; source 0 is exactly zero over the first third of signal 0."""
    img = levelled((S, n_sig, L), 1000 * n_fft + 100 * S + T + (pad == 'reflect'))
    img[0, 0, :L // 3] = 0
    assert 1 + L // (n_fft // 2) == T
    hop = n_fft // 2
    x64 = img.astype(np.float64)
    st = lambda x: np.swapaxes(so.stft(x, n_fft, hop, pad, np.complex128), -1, -2)          # (..., T, F)
    total = x64[0].copy()
    for j in range(1, S):
        total = total + x64[j]
    norms = sum(np.linalg.norm(mc._frames(img[j], n_fft, pad, np.float64), axis=-1) for j in range(S))
    delta = (U * np.sqrt(n_fft) * norms)[..., None]                           # (n_sig, T, 1)
    X32 = [scipy.fft.rfft(mc._frames(img[j], n_fft, pad, np.float32), axis=-1) for j in range(S)]
    assert X32[0].dtype == np.complex64
    mix32 = X32[0].copy()
    for j in range(1, S):
        mix32 = mix32 + X32[j]
    mix_ref = st(total)
    out = {'img': img, 'delta': delta, 'mix': mix_ref, 'mix_f32_ratio': float(np.max(np.abs(mix32 - mix_ref) / delta)), 'kinds': {}}
    per_source = []
    for i in range(S):
        others = [j for j in range(S) if j != i]
        n64 = x64[others[0]].copy()
        N32 = X32[others[0]].copy()
        for j in others[1:]:
            n64 = n64 + x64[j]
            N32 = N32 + X32[j]
        assert N32.dtype == np.complex64
        per_source.append((st(x64[i]), st(n64), X32[i], N32))
    for kind in MASK_KINDS:
        ibm = kind.startswith('ibm')
        ref, f32, G, clear, zero = [], [], [], [], []
        for Si, Ni, S32, N32 in per_source:
            aS, aN, aY = np.abs(Si), np.abs(Ni), np.abs(Si + Ni)
            with np.errstate(all='ignore'):
                ref.append(np.asarray(mo.tf_mask(Si, Ni, kind), np.float64))
                f32.append(np.asarray(mo.tf_mask(S32, N32, kind), np.float64))
            G.append(mc._sens(aS, aN, aY, kind, (4 if ibm else C_MEETING) * delta))
            if ibm:
                xi = (aS / np.maximum(aN, mc.EPS)) ** int(kind[3])
                clear.append(np.abs(xi - 1.0) > 4 * delta * G[-1])
                zero.append(aN == 0)
        rec = {'ref': np.stack(ref), 'f32': np.stack(f32), 'G': np.stack(G)}
        if ibm:
            rec['clear'], rec['zero'] = np.stack(clear), np.stack(zero)
            rec['band'] = float(np.mean(~rec['clear'] & ~rec['zero']))
            assert np.array_equal(rec['f32'][rec['clear']], rec['ref'][rec['clear']]), 'the float32 restatement decides like the oracle outside the band'
        else:
            fin = np.isfinite(rec['ref'])
            assert np.array_equal(np.isnan(rec['f32']), ~fin), 'the float32 restatement is NaN where the oracle is, and nowhere else'
            dG = np.broadcast_to(delta, rec['ref'].shape) * rec['G']
            rec['f32_ratio'] = mc._worst_ratio(np.abs(rec['f32'][fin] - rec['ref'][fin]), rec['ref'][fin], dG[fin])
        out['kinds'][kind] = rec
    return out


def f32_restatement_ratio(cases=None):
    """The worst err / (delta G) of the float32 restatement over the value kinds of every case: C_MEETING is 4 x this."""
    return max(mask_case(*c)['kinds'][k]['f32_ratio'] for c in (cases or mask_cases()) for k in VALUE_KINDS)


def ibm_band_fraction(cases=None):
    return max(mask_case(*c)['kinds']['ibm1']['band'] for c in (cases or mask_cases()))


def check_mask_case(make_engine, case, kinds=MASK_KINDS):
    """Every bin of every frame of every source, and the mix spectrum.  -> the kernel's worst err / (delta G) over the value kinds."""
    n_fft, pad, S, T, L, n_sig = case
    ref = mask_case(*case)
    worst = 0.0
    for kind in kinds:
        eng = make_engine(rooms=n_sig, nodes=1, mics=1, length=L, n_fft=n_fft, mask=kind, pad_mode=pad)
        assert (eng.T, eng.F) == (T, n_fft // 2 + 1)
        masks, mix = eng.source_masks(ref['img'])
        m, mix = masks.numpy().astype(np.float64), mix.numpy()
        assert m.shape == (S, n_sig, T, eng.F) and mix.shape == (n_sig, T, eng.F) and mix.dtype == np.complex64
        e_mix = np.abs(mix - ref['mix'])
        assert np.all(e_mix <= C_MEETING * ref['delta']), f'{case}: mix spectrum, worst err / delta {float((e_mix / ref["delta"]).max()):.3g}'
        _same_bits(eng.source_masks(ref['img'], want_mix=False)[0].numpy(), masks.numpy(), f'{case} {kind}: masks without the mix')
        rec = ref['kinds'][kind]
        if kind.startswith('ibm'):
            assert np.all((m == 0) | (m == 1))
            bad = (rec['clear'] & ~rec['zero'] & (m != rec['ref'])) | (rec['zero'] & (m != rec['f32']))
            assert not bad.any(), f'{case} {kind}: {int(bad.sum())} wrong decisions outside the band, first at {np.argwhere(bad)[0]}'
            continue
        fin = np.isfinite(rec['ref'])
        assert np.array_equal(np.isnan(m), np.isnan(rec['ref'])) and np.array_equal(np.isinf(m), np.isinf(rec['ref'])), \
            f'{case} {kind}: NaN / inf where the oracle has them ({int((~fin).sum())} bins) and nowhere else'
        err = np.where(fin, np.abs(m - np.where(fin, rec['ref'], 0)), 0)
        dG = np.where(fin, ref['delta'] * rec['G'], 1)
        bar = C_MEETING * dG + 4 * U * np.abs(np.where(fin, rec['ref'], 0))
        ratio = float(mc._worst_ratio(err[fin], rec['ref'][fin], dG[fin]))
        print(f'meeting masks {case} {kind}: kernel worst err / (delta G) {ratio:.4g}, mix worst err / delta {float((e_mix / ref["delta"]).max()):.4g}')
        bad = err > bar
        assert not bad.any(), f'{case} {kind}: {int(bad.sum())} of {bad.size} bins beyond the bar, worst err / bar {float((err / bar)[bad].max()):.3g}, first at {np.argwhere(bad)[0]}'
        worst = max(worst, ratio)
    return worst


def check_mask_lengths(make_engine, n_fft=512, pad='reflect', S=3, n_mic=2, kind='irm1'):
    """A batch with set_lengths equals each room run alone at its own length, bit for bit; zeros in the frames beyond each length; NaN
    planted beyond each length is never read.  The rooms: the whole clip, the shortest legal length, one in between."""
    hop = n_fft // 2
    Lmax = 18 * hop + 77
    lengths = np.array([Lmax, hop + 1 if pad == 'reflect' else 1, 16 * hop + 5], np.int32)
    R = len(lengths)
    img = levelled((S, R, n_mic, Lmax), n_fft + S)
    for r in range(R):
        img[:, r, :, lengths[r]:] = np.nan
    eng = make_engine(rooms=R, nodes=1, mics=n_mic, length=Lmax, n_fft=n_fft, mask=kind, pad_mode=pad)
    eng.set_lengths(lengths)
    masks, mix = (a.numpy() for a in eng.source_masks(img.reshape(S, R * n_mic, Lmax)))
    eng.set_lengths(None)
    masks, mix = masks.reshape(S, R, n_mic, eng.T, eng.F), mix.reshape(R, n_mic, eng.T, eng.F)
    for r in range(R):
        Lr = int(lengths[r])
        Tr = 1 + Lr // hop
        solo = make_engine(rooms=1, nodes=1, mics=n_mic, length=Lr, n_fft=n_fft, mask=kind, pad_mode=pad)
        m1, x1 = (a.numpy() for a in solo.source_masks(np.ascontiguousarray(img[:, r, :, :Lr])))
        assert np.isfinite(m1).all() and np.isfinite(x1).all(), r
        _same_bits(masks[:, r, :, :Tr], m1, f'{n_fft} {pad} room {r} (length {Lr}): masks')
        _same_bits(mix[r, :, :Tr], x1, f'{n_fft} {pad} room {r} (length {Lr}): mix')
        assert not masks[:, r, :, Tr:].any() and not mix[r, :, Tr:].any(), f'room {r}: zeros in the frames beyond its length'
        assert not np.signbit(masks[:, r, :, Tr:]).any()
    _refused(lambda: (eng.set_lengths(lengths), eng.source_masks(img.reshape(S, R * n_mic, Lmax)[:, :R * n_mic - 1]))[1], 'multiple of cfg.rooms',
             _disco_error())
    eng.set_lengths(None)


def _disco_error():
    from disco_amd.engine import DiscoError
    return DiscoError


def check_mask_batch_independence(make_engine, n_fft=512, S=5, n_sig=6, T=18):
    """A signal inside a batch equals the same signal alone, bit for bit (masks and mix); the outputs do not depend on what a call before
    left in the wave's exchange buffer either (two different batches in turn)."""
    hop = n_fft // 2
    L = (T - 1) * hop + 31
    img = levelled((S, n_sig, L), 77)
    eng = make_engine(rooms=n_sig, nodes=1, mics=1, length=L, n_fft=n_fft, mask='irm1')
    masks, mix = (a.numpy() for a in eng.source_masks(img))
    solo = make_engine(rooms=1, nodes=1, mics=1, length=L, n_fft=n_fft, mask='irm1')
    for g in (0, 3, n_sig - 1):
        m1, x1 = (a.numpy() for a in solo.source_masks(np.ascontiguousarray(img[:, g:g + 1])))
        _same_bits(masks[:, g:g + 1], m1, f'signal {g} alone: masks')
        _same_bits(mix[g:g + 1], x1, f'signal {g} alone: mix')
    again = [a.numpy() for a in eng.source_masks(np.ascontiguousarray(img[:, ::-1]))]
    _same_bits(again[0][:, ::-1], masks, 'the batch in reverse order: masks')
    _same_bits(again[1][::-1], mix, 'the batch in reverse order: mix')


def check_mask_refusals(make_engine):
    """S = 1 and S = 9 are refused with the limit named; nothing is written and the context stays usable."""
    from disco_amd import _lib
    L = 1024
    eng = make_engine(rooms=2, nodes=1, mics=1, length=L, n_fft=512)
    img = levelled((9, 2, L), 4)
    pi, ki = eng.to_device(img, np.float32)
    sent_m, sent_x = np.full((9, 2, eng.T, eng.F), 7.0, np.float32), np.full((2, eng.T, eng.F), 7.0 + 7.0j, np.complex64)
    (pm, km), (px, kx) = eng.to_device(sent_m, np.float32), eng.to_device(sent_x, np.complex64)
    for S in (1, 9, 0, -2):
        assert eng.lib.disco_source_masks(eng.ctx, pi, S, 2, pm, px, eng.stream) == _lib.E_UNSUPPORTED, S
        assert '2 <= n_src <= 8' in eng.lib.disco_last_error(eng.ctx).decode()
    assert eng.lib.disco_source_masks(eng.ctx, None, 2, 2, pm, px, eng.stream) == _lib.E_ARG
    assert eng.lib.disco_source_masks(eng.ctx, pi, 2, 2, None, px, eng.stream) == _lib.E_ARG
    assert eng.lib.disco_source_masks(eng.ctx, pi, 2, 0, pm, px, eng.stream) == _lib.E_ARG
    eng.sync()
    _same_bits(km.numpy(), sent_m, 'masks after the refusals')
    _same_bits(kx.numpy(), sent_x, 'mix after the refusals')
    assert eng.lib.disco_source_masks(eng.ctx, pi, 8, 2, pm, px, eng.stream) == 0
    got = km.numpy()
    _same_bits(got[:8], eng.source_masks(img[:8])[0].numpy(), 'the same buffers are then taken')
    _same_bits(got[8], sent_m[8], 'the ninth block stays untouched')
    _refused(lambda: eng.source_masks(img[:1]), '2 <= n_src <= 8', _disco_error())
    _refused(lambda: eng.source_masks(img), '2 <= n_src <= 8', _disco_error())


# ---- the Python layer (the package's own engine) ---------------------------------------------------------------------------------------------
def _package_engine():
    from disco_amd._engines import get_engine
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)


def sir_scene(S, mics_per_node, R=2, L=3000, seed=31):
    img = levelled((S, R, sum(mics_per_node), L), seed)
    # every node hears its own talker best (as a node next to its talker does), by a margin drawn per node
    rng = np.random.default_rng(seed)
    edges = np.concatenate([[0], np.cumsum(mics_per_node)])
    for k in range(S):
        rms = np.sqrt(np.mean(img[:, :, edges[k]:edges[k + 1]].astype(np.float64) ** 2, axis=(1, 2, 3)))
        img[k, :, edges[k]:edges[k + 1]] *= np.float32(rms.max() / rms[k] * 10 ** rng.uniform(0.1, 0.6))
    return img


def _node_pair(img, k, r, c):
    """Channel c of room r as node k hears it: its own talker, the float32 sum of the others in ascending order, and their sum."""
    others = [j for j in range(img.shape[0]) if j != k]
    n = img[others[0], r, c].copy()
    for j in others[1:]:
        n = n + img[j, r, c]
    return img[k, r, c], n, img[k, r, c] + n


def sir_by_hand(img, mics_per_node, stop=None):
    """sir_at_node (the reference's, convolve_signals.py:81-91) through metrics.bss_eval_sources on NumPy sums, one (node, microphone) at a time."""
    from disco_amd import metrics as dm
    S, R, n_mic, L = img.shape
    edges = np.concatenate([[0], np.cumsum(mics_per_node)])
    out = np.zeros((R, S))
    for r in range(R):
        st = L if stop is None else int(stop[r])
        for k in range(S):
            sirs = []
            for c in range(edges[k], edges[k + 1]):
                s, n, m = _node_pair(img, k, r, c)
                sirs.append(dm.bss_eval_sources(np.stack([s, n]), np.stack([m, m]), compute_permutation=False, stop=st)[1][0])
            out[r, k] = np.mean(sirs)
    return out


def check_sir_at_nodes(cases=((2, (2, 2)), (3, (1, 2, 1)), (4, (1, 1, 1, 1))), L=3000, R=2):
    """Against metrics.bss_eval_sources called by hand on NumPy sums, bit for bit (NumPy and device-resident images, with and without a
    stop per room), and against the float64 Gram oracle of tests/bss_checks.py at its TOL_DB."""
    import bss_checks as bc
    from disco_amd.dataset_utils import sir_at_nodes
    eng = _package_engine()
    for S, mpn in cases:
        img = sir_scene(S, mpn, R=R, L=L, seed=30 + S)
        got = sir_at_nodes(img, mpn)
        assert got.shape == (R, S) and got.dtype == np.float64
        _same_bits(got, sir_by_hand(img, mpn), f'S {S}, nodes {mpn}: SIRs against the calls made by hand')
        _same_bits(sir_at_nodes(eng.to_device(img, np.float32)[1], mpn), got, f'S {S}: device-resident images')
        stop = np.array([L - 700, L])[:R]
        dirty = img.copy()
        dirty[:, 0, :, stop[0]:] = np.nan
        _same_bits(sir_at_nodes(dirty, mpn, stop=stop), sir_by_hand(img, mpn, stop), f'S {S}: a stop per room')
        edges = np.concatenate([[0], np.cumsum(mpn)])
        worst = 0.0
        for r in range(R):
            for k in range(S):
                vals = []
                for c in range(edges[k], edges[k + 1]):
                    s, n, m = _node_pair(img, k, r, c)
                    vals.append(bc.gram_oracle(np.stack([s, n]), m, 0, 512)[1])
                assert np.mean(vals) <= 40.0
                worst = max(worst, abs(got[r, k] - np.mean(vals)))
        print(f'meeting sir_at_nodes S={S} nodes={mpn}: SIRs {np.round(got, 3).tolist()}, worst |err| against the float64 oracle {worst:.3g} dB')
        assert worst < bc.TOL_DB, (S, worst)
    _refused(lambda: sir_at_nodes(sir_scene(3, (1, 2, 1)), (2, 2)), 'need 3 nodes')
    _refused(lambda: sir_at_nodes(sir_scene(2, (2, 2)), (2, 1)), 'add up')
    _refused(lambda: sir_at_nodes(sir_scene(2, (2, 2))[0], (2, 2)), 'source-major')


def check_sir_valid_golden():
    """sir_valid and get_value_range against the reference's own functions (tests/golden/meeting_ref.npz)."""
    from disco_amd.dataset_utils import get_value_range, sir_valid
    from disco_amd.dataset_utils.meetings import sir_classes
    fx = fixture()
    names = sorted(k[5:] for k in fx if k.startswith('sirs_'))
    assert len(names) >= 10
    for name in names:
        sirs, want = fx[f'sirs_{name}'], fx[f'valid_{name}']
        n_rirs, delta = (int(v) for v in fx[f'args_{name}'])
        valid, past = sir_valid(sirs, n_rirs, delta_sir=delta)
        assert valid.dtype == bool and np.array_equal(valid, want), (name, valid, want)
        assert len(past) == sirs.shape[1] and np.array_equal(np.array(past[0]), fx[f'past0_{name}']), name
        assert np.array_equal(np.array(past).T, sirs[want]), name
        # judged in two halves with the history handed on: the same verdicts (and the caller's history is not modified)
        h = len(sirs) // 2
        v1, p1 = sir_valid(sirs[:h], n_rirs, delta_sir=delta)
        kept = [list(p) for p in p1]
        v2, p2 = sir_valid(sirs[h:], n_rirs, past=p1, delta_sir=delta)
        assert np.array_equal(np.concatenate([v1, v2]), want) and p1 == kept and p2 == past, name
    starts, stops, level = sir_classes(10)
    assert np.array_equal(np.stack([starts, stops], axis=1), fx['class_edges']) and np.all(fx['class_level_n10'] == level)
    for args, want in zip(fx['gvr_args'], fx['gvr_out']):
        i, n, vmin, vmax, nb = args
        got = get_value_range(int(i), int(n), vmin, vmax, int(nb))
        assert isinstance(got, np.ndarray) and np.array_equal(got, want), (args, got, want)
    assert np.array_equal(get_value_range(3, 10), get_value_range(3, 10, 0, 20, 5))
    _refused(lambda: sir_valid(np.zeros(3), 4), '(R, S)')
    _refused(lambda: sir_valid(np.zeros((2, 3)), 4, past=[[], []]), 'one list per source')


ROOM_KW = dict(fs=16000, max_order=3, rir_len=512)


def meeting_scene(R, S, mics_per_node, Ld=2500, seed=60):
    rng = np.random.default_rng(seed)
    n_mic = sum(mics_per_node)
    dims = np.array([[4.0, 5.0, 3.0], [5.5, 4.2, 2.8], [6.0, 3.5, 3.1]], np.float32)[:R]
    absorption = np.array([0.35, 0.5, 0.25], np.float32)[:R]
    src = (dims[:, None, :] * rng.uniform(0.2, 0.8, (R, S, 3))).astype(np.float32)
    mic = (dims[:, None, :] * rng.uniform(0.15, 0.85, (R, n_mic, 3))).astype(np.float32)
    dry = np.moveaxis(levelled((S, R, Ld), seed + 1), 0, 1)
    return np.ascontiguousarray(dry), dims, absorption, src, mic


def check_simulate_meetings(R=2, S=3, mics_per_node=(1, 2, 1), Ld=2500, out_len=3300):
    """simulate_meetings == the same public calls made by hand.  The RIRs against the float64 ISM oracle at 5e-6 of the largest tap;
    everything downstream bit for bit from the returned RIRs; the images within 2e-6 of np.convolve (zero-padded to out_len)."""
    from disco_amd.dataset_utils import simulate_meetings, sir_at_nodes
    from disco_amd.engine import DevBuf
    from oracle import ism_oracle as io
    dry, dims, absorption, src, mic = meeting_scene(R, S, mics_per_node, Ld)
    n_mic = sum(mics_per_node)
    assert Ld + 511 < out_len, 'the images are padded beyond the end of the convolution'
    lengths = np.array([out_len, out_len - 400])[:R]
    res = simulate_meetings(dry, dims, absorption, src, mic, mics_per_node, out_len=out_len, lengths=lengths, **ROOM_KW)
    assert set(res) == {'images', 'rirs', 'sirs'} and isinstance(res['images'], DevBuf) and isinstance(res['rirs'], DevBuf)
    img, rir = res['images'].numpy(), res['rirs'].numpy()
    assert img.shape == (S, R, n_mic, out_len) and rir.shape == (S, R, n_mic, 512) and res['sirs'].shape == (R, S)
    e_rir = max(float(np.max(np.abs(rir[i, r, c] - (want := io.ism_rir(dims[r], float(absorption[r]), src[r, i], mic[r, c], 3, 16000.0, 343.0, 512)))) /
                      np.max(np.abs(want))) for i in range(S) for r in range(R) for c in range(n_mic))
    print('meeting simulate_meetings, RIRs against the float64 oracle:', e_rir)
    assert e_rir < 5e-6, e_rir
    eng = _package_engine()
    by_hand = eng.rir_convolve(np.ascontiguousarray(np.swapaxes(dry, 0, 1)).reshape(S * R, Ld), rir.reshape(S * R, n_mic, 512), out_len=out_len).numpy()
    _same_bits(img, by_hand.reshape(img.shape), 'images')
    _same_bits(res['sirs'], sir_at_nodes(img, mics_per_node, stop=lengths), 'sirs')
    worst = 0.0
    for i in range(S):
        for r in range(R):
            for c in range(n_mic):
                want = np.zeros(out_len)
                full = np.convolve(dry[r, i].astype(np.float64), rir[i, r, c].astype(np.float64))
                want[:min(out_len, full.size)] = full[:out_len]
                worst = max(worst, float(np.max(np.abs(img[i, r, c] - want)) / np.max(np.abs(want))))
    print('meeting simulate_meetings, images against np.convolve:', worst)
    assert worst < 2e-6, worst                                               # (beyond Ld + rir_len - 1, the pad to len_max, `want` is zero)
    cut = simulate_meetings(eng.to_device(dry, np.float32)[1], dims, absorption, src, mic, mics_per_node, out_len=Ld - 500, **ROOM_KW)    # device in, truncated
    assert cut['images'].shape == (S, R, n_mic, Ld - 500)
    by_hand = eng.rir_convolve(np.ascontiguousarray(np.swapaxes(dry, 0, 1)).reshape(S * R, Ld), cut['rirs'].reshape(S * R, n_mic, 512), out_len=Ld - 500)
    _same_bits(cut['images'].numpy().reshape(by_hand.shape), by_hand.numpy(), 'images from device-resident sources, truncated')
    _refused(lambda: simulate_meetings(dry, dims, absorption, src, mic, (2, 2), **ROOM_KW), 'need 3 nodes')
    _refused(lambda: simulate_meetings(dry, dims, absorption, src[:, :2], mic, mics_per_node, **ROOM_KW), 'src_pos')
    _refused(lambda: simulate_meetings(dry[0], dims, absorption, src, mic, mics_per_node, **ROOM_KW), '(R, S, Ld)')
    return res


def check_meeting_rooms_tango(R=2, L=4096, lengths=(4096, 3000)):
    """meeting_rooms (K = S = 2, M = 2) -> offline_tango_batched on the device-resident (y, s, n) == the same call on their host copies,
    with and without lengths; (y, s, n) bit for bit the NumPy sums."""
    from disco_amd.dataset_utils import meeting_rooms
    from disco_amd.engine import DevBuf
    from disco_amd.speech_enhancement.tango import offline_tango_batched
    rng = np.random.default_rng(12)
    # two talkers through short random filters, so that the channels of a node are coherent and the spatial filters have something to do
    dry = levelled((2, R, L + 32), 13)
    img = np.zeros((2, R, 4, L), np.float32)
    for i in range(2):
        for r in range(R):
            for c in range(4):
                h = rng.standard_normal(24) * np.exp(-np.arange(24) / 5.0) * (1.0 if c // 2 == i else 0.4)
                img[i, r, c] = np.convolve(dry[i, r], h)[24:24 + L]
    img += (1e-3 * rng.standard_normal(img.shape)).astype(np.float32)
    for lens in (None, np.array(lengths[:R], np.int32)):
        y, s, n = meeting_rooms(img, (2, 2), lengths=lens)
        assert all(isinstance(a, DevBuf) and a.shape == (R, 2, 2, L) for a in (y, s, n))
        yh, sh, nh = y.numpy(), s.numpy(), n.numpy()
        ref = mix_reference(img, np.array([0, 0, 1, 1]), None if lens is None else lens[:, None])
        for name, g, w in zip('ysn', (yh, sh, nh), ref):
            _same_bits(g.reshape(w.shape), w, f'lengths {lens}: {name}')
        dev = offline_tango_batched(y, s, n, lengths=lens)
        host = offline_tango_batched(yh, sh, nh, lengths=lens)
        assert set(dev) == set(host) and 'yf' in dev
        for k in dev:
            _same_bits(dev[k], host[k], f'lengths {lens}: offline_tango_batched[{k}] on the device-resident rooms')
        assert np.isfinite(dev['yf']).all() and np.abs(dev['yf']).max() > 0
    _refused(lambda: meeting_rooms(img, (3, 1)), '[3, 1]')
    _refused(lambda: meeting_rooms(img, (1, 1, 1, 1)), 'need 2 nodes')
    _refused(lambda: meeting_rooms(img, (2, 2), lengths=[1, 2, 3]), 'per room')


def check_meeting_masks(make_engine, n_fft=512, T=17, n_mic=3):
    """meeting_masks == Engine.source_masks (with and without lengths); for S = 2 its masks also lie inside the bar that
    mask_metric_checks.check_oracle_case holds Engine.mask_oracle(img_i, img_other) to."""
    from disco_amd.dataset_utils import meeting_masks
    from disco_amd.engine import DevBuf
    hop = n_fft // 2
    R, L = 2, (T - 1) * hop + 19
    for S, kind in ((2, 'irm1'), (5, 'iam1')):
        img = levelled((S, R, n_mic, L), 40 + S)
        for lens in (None, np.array([L, L - 3 * hop - 7], np.int32)):
            stfts, masks = meeting_masks(img, mics_per_node=(1, n_mic - 1), lengths=lens, type=kind, n_fft=n_fft)
            assert isinstance(stfts, DevBuf) and stfts.shape == (R, n_mic, T, hop + 1) and masks.shape == (S, R, n_mic, T, hop + 1)
            eng = make_engine(rooms=R, nodes=1, mics=n_mic, length=L, n_fft=n_fft, mask=kind)
            eng.set_lengths(lens)
            m, x = eng.source_masks(img.reshape(S, R * n_mic, L))
            _same_bits(masks.numpy().reshape(m.shape), m.numpy(), f'S {S}, lengths {lens}: masks')
            _same_bits(stfts.numpy().reshape(x.shape), x.numpy(), f'S {S}, lengths {lens}: stfts')
        if S == 2:                                                           # the existing bar of the two-signal oracle mask, per source
            got = meeting_masks(img, type=kind, n_fft=n_fft)[1].numpy().astype(np.float64).reshape(2, R * n_mic, T, hop + 1)
            for i in range(2):
                s, n = img[i].reshape(R * n_mic, L), img[1 - i].reshape(R * n_mic, L)
                Sf = np.swapaxes(so.stft(s, n_fft, hop, 'reflect', np.complex128), -1, -2)
                Nf = np.swapaxes(so.stft(n, n_fft, hop, 'reflect', np.complex128), -1, -2)
                delta = (U * np.sqrt(n_fft) * (np.linalg.norm(mc._frames(s, n_fft, 'reflect', np.float64), axis=-1) +
                                                np.linalg.norm(mc._frames(n, n_fft, 'reflect', np.float64), axis=-1)))[..., None]
                ref = np.asarray(mo.tf_mask(Sf, Nf, kind), np.float64)
                G = mc._sens(np.abs(Sf), np.abs(Nf), np.abs(Sf + Nf), kind, mc.C_ORACLE * delta)
                err = np.abs(got[i] - ref)
                assert np.all(err <= mc.C_ORACLE * delta * G + 4 * U * np.abs(ref)), (i, float((err / (mc.C_ORACLE * delta * G + 4 * U * np.abs(ref))).max()))
    _refused(lambda: meeting_masks(img, mics_per_node=(2, 2)), 'add up')
    _refused(lambda: meeting_masks(img[0]), 'source-major')
    _refused(lambda: meeting_masks(img, type='xyz1'), 'Unknown mask type')
