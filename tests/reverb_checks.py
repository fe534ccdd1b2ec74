"""Checks of the reverberation ratios (disco_rir_split, disco_reverb_energies, csrc/k_reverb.h; disco_amd.metrics.reverb_ratios and
dataset_utils.rooms.reverb_at_mics), shared by tests/test_levels_emulated.py (hipemu) and tests/test_gpu_levels.py (MI355X).

The yardstick is tests/golden/levels_ref.npz: the reference's own reverb_ratios (np.argmax, two float64 np.convolve calls) run on float64
copies of the float32 inputs (tests/golden/make_golden_levels.py, whose case tables are imported here); where the reference cannot answer
(an empty direct part or tail makes its np.convolve raise) the definition is restated in float64 NumPy below.

Bars, derived and not taken from the code under test:
  TOL_DRR = 1e-10 dB   DRR and the energies of disco_rir_split: the squares of float32 values are exact in float64 and a sum of n <= 8192
                       terms is within n 2^-53.
  split                exact.
  TOL_SRR = 3.5e-5 dB  = 4 eps 10 / ln 10 with eps = 2e-6, the relative l2 bar parity_checks.check_rir_convolve holds this convolution
                       scheme to: each convolution within eps, each energy within 2 eps, their ratio within 4 eps.
  4 eps relative       the first energy at split == rir_len against the summed squares of Engine.rir_convolve's full-length output;
                       the second energy is then an exact 0.
Measured (lines starting `levels `), the same figures on the MI355X and under hipemu: DRR worst 5.0e-14 dB; SRR worst 7.1e-7 dB over the
78 golden pairs (SRR -39 .. 84 dB; 2.6e-7 .. 7.1e-7 per shape); energy against rir_convolve worst 2.2e-16 relative (the same
arithmetic, summed in another order); rir_split energies against float64 NumPy worst 1.9e-15 dB.
"""
import os

import numpy as np
import pytest

import segsnr_checks as sg

gen = sg.gen
HERE = os.path.dirname(os.path.abspath(__file__))
EPS_CONV = 2e-6
TOL_DRR = 1e-10
TOL_SRR = 4 * EPS_CONV * 10 / np.log(10)
FS = gen.FS


def _eng():
    from disco_amd import metrics as dm
    return dm._engine()


def n_direct(reverb_start):
    return int(1e-3 * reverb_start * FS)


def split_def(rir, n_d):
    """the definition: np.argmax of the signed response (first maximum; a NaN wins at its first index) + n_d, capped at rir_len"""
    return np.minimum(np.argmax(rir, axis=-1) + n_d, rir.shape[-1]).astype(np.int32)


def tap_energies_def(rir, split):
    h = rir.astype(np.float64).reshape(-1, rir.shape[-1])
    sp = np.asarray(split).reshape(-1)
    e = np.array([[np.sum(h[i, :sp[i]] ** 2), np.sum(h[i, sp[i]:] ** 2)] for i in range(len(sp))])
    return e.reshape(tuple(np.shape(split)) + (2,))


def _db_close(got, want, tol):
    """energies: exact where the yardstick is 0, NaN where it is NaN, within tol dB elsewhere -> worst |dB|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[want == 0], want[want == 0])
    ok = ~np.isnan(want) & (want != 0)
    worst = float(np.max(np.abs(10 * np.log10(got[ok] / want[ok])))) if ok.any() else 0.0
    assert worst < tol, (worst, tol)
    return worst


def golden_shape(k):
    g = sg.golden()
    x, rir, rs, kinds = gen.reverb_inputs(k)
    assert np.array_equal(g[f'rev{k}_x'], x) and np.array_equal(g[f'rev{k}_rir'], rir) and np.array_equal(g[f'rev{k}_start'], rs)
    return x, rir, rs, kinds, g[f'rev{k}_drr'], g[f'rev{k}_srr']


def device_splits(eng, rir, rs):
    """disco_rir_split with the n_direct of every pair (one call per distinct value) -> split (n_sig, n_ch) int32, energy (n_sig, n_ch, 2)"""
    split = np.zeros(rs.shape, np.int32)
    energy = np.zeros(rs.shape + (2,))
    for v in np.unique(rs):
        sp, en = eng.rir_split(rir, n_direct(v))
        split[rs == v], energy[rs == v] = sp.numpy()[rs == v], en.numpy()[rs == v]
    return split, energy


def check_golden(k):
    """One shape of the fixture: the split exact, DRR and SRR of all pairs in one batch against the reference's values; the rows alone
    (n_sig = 1, n_ch = 1) have the bits they have in the batch; a few pairs through the 1-D Python surface."""
    from disco_amd import metrics as dm
    x, rir, rs, kinds, drr, srr = golden_shape(k)
    Ld, Lh, n_sig, n_ch = gen.REVERB_SHAPES[k]
    eng = _eng()
    split, e_h = device_splits(eng, rir, rs)
    want_split = np.array([[split_def(rir[i, c], n_direct(rs[i, c])) for c in range(n_ch)] for i in range(n_sig)])
    assert np.array_equal(split, want_split) and np.all((split > 0) & (split < Lh))
    for i in range(n_sig):
        for c in range(n_ch):
            assert split[i, c] == gen.split_plan(gen.SPLIT_KINDS[kinds[i, c]], Lh)[2]
    _db_close(e_h, tap_energies_def(rir, split), TOL_DRR)
    worst_drr = float(np.max(np.abs(dm._ratio_db(e_h) - drr)))
    e_x = eng.reverb_energies(x, rir, split).numpy()
    assert np.array_equal(e_x, eng.reverb_energies(x, rir, split).numpy())                     # run to run
    got_srr = dm._ratio_db(e_x)
    worst_srr = float(np.max(np.abs(got_srr - srr)))
    print(f'levels reverb golden Ld {Ld} rir_len {Lh}: {n_sig * n_ch} pairs, splits {sorted(set(split.reshape(-1).tolist()))}, SRR {srr.min():.1f} .. '
          f'{srr.max():.1f} dB, worst |DRR diff| = {worst_drr:.3g} dB (bar {TOL_DRR:g}), worst |SRR diff| = {worst_srr:.3g} dB (bar {TOL_SRR:.3g})')
    assert worst_drr < TOL_DRR and worst_srr < TOL_SRR
    for i in range(n_sig):                                                                     # alone: one signal, one channel
        for c in range(n_ch):
            alone = eng.reverb_energies(x[i:i + 1], rir[i:i + 1, c:c + 1].copy(), split[i:i + 1, c:c + 1].copy()).numpy()
            assert np.array_equal(alone[0, 0], e_x[i, c]), (i, c, alone, e_x[i, c])
    if n_sig > 1:                                                                              # one signal with all its channels
        assert np.array_equal(eng.reverb_energies(x[1:2], rir[1:2], split[1:2]).numpy()[0], e_x[1])
    for i, c in ((0, 0), (n_sig - 1, n_ch - 1)):                                               # the reference's own call
        d1, s1 = dm.reverb_ratios(x[i], rir[i, c], reverb_start=rs[i, c], fs=FS)
        assert isinstance(d1, float) and isinstance(s1, float)
        assert d1 == dm._ratio_db(e_h)[i, c] and s1 == got_srr[i, c]
    return worst_drr, worst_srr


def check_special_rows():
    """The two rows of the (1500, 1300) shape that were built to catch something: the tail's energy past the end of the dry signal (a
    dropped trailing block would miss the bar by orders of magnitude) and a direct path 40 dB above the tail."""
    x, rir, rs, kinds, drr, srr = golden_shape(2)
    Ld, Lh = x.shape[1], rir.shape[2]
    h_r = rir[0, 0].astype(np.float64).copy()
    h_r[:1] = 0.0
    tail = np.convolve(x[0].astype(np.float64), h_r)
    n_blocks = -(-(Ld + Lh - 1) // 512)
    last = np.sum(tail[(n_blocks - 1) * 512:] ** 2) / np.sum(tail ** 2)
    past = np.sum(tail[Ld:] ** 2) / np.sum(tail ** 2)
    print(f'levels reverb tail case: {past:.3f} of the tail energy past the dry signal, {last:.3f} in the last block; 40 dB case: DRR {drr[1, 1]:.2f} SRR {srr[1, 1]:.2f} dB')
    assert past > 0.5 and 10 * np.log10(1 / (1 - last)) > 1e3 * TOL_SRR                      # dropping the last block alone: 0.23 dB
    assert abs(drr[1, 1] - 40.0) < 1e-6 and 35 < srr[1, 1] < 45


def check_full_tail_against_rir_convolve():
    """split == rir_len on every shape of the list: the second energy is an exact 0 and the first equals the summed squares of
    Engine.rir_convolve's full-length output within 4 eps relative; reverb_ratios then gives +inf for both."""
    from disco_amd import metrics as dm
    eng = _eng()
    rng = np.random.default_rng(77)
    worst = 0.0
    for Ld, Lh, _, _ in gen.REVERB_SHAPES:
        n_sig, n_ch = (1, 2) if Lh > 4096 else (2, 2)
        x = rng.standard_normal((n_sig, Ld)).astype(np.float32)
        rir = (rng.standard_normal((n_sig, n_ch, Lh)) * np.exp(-np.arange(Lh) / (0.3 * Lh))).astype(np.float32)
        e = eng.reverb_energies(x, rir, np.full((n_sig, n_ch), Lh, np.int32)).numpy()
        y = eng.rir_convolve(x, rir, out_len=Ld + Lh - 1).numpy().astype(np.float64)
        want = np.sum(y ** 2, axis=-1)
        rel = float(np.max(np.abs(e[..., 0] - want) / want))
        worst = max(worst, rel)
        assert np.all(e[..., 1] == 0.0) and rel < 4 * EPS_CONV, (Ld, Lh, rel, e)
        rir[..., Lh - 1] = 9.0                                                                 # the peak at the last tap: an empty tail
        drr, srr = dm.reverb_ratios(x, rir)
        assert drr.shape == (n_sig, n_ch) and np.all(drr == np.inf) and np.all(srr == np.inf)
    print(f'levels reverb energy against rir_convolve at split == rir_len: worst relative diff = {worst:.3g} (bar {4 * EPS_CONV:g})')


def split_cases(Lh=700):
    """-> rir (7, Lh): peak at 0; peak at rir_len - 1; two equal maxima (the first wins); a negative tap of larger magnitude than the
    maximum; a NaN row (two NaNs, the first wins, a larger value before it) between clean rows; a plain row; all taps equal."""
    rng = np.random.default_rng(5)
    h = (0.3 * rng.standard_normal((7, Lh)) * np.exp(-np.arange(Lh) / 150.0)).clip(-0.8, 0.8)
    h[0, 0] = 1.0
    h[1, Lh - 1] = 1.0
    h[2, 300] = h[2, 77] = 0.9
    h[3, 50], h[3, 10] = 0.85, -3.0
    h[4, 20], h[4, 130], h[4, 400] = 2.0, np.nan, np.nan
    h[5, 257] = 1.5
    h[6] = 0.25
    return h.astype(np.float32)


def check_rir_split():
    from disco_amd import metrics as dm
    eng = _eng()
    h = split_cases()
    Lh = h.shape[1]
    worst = 0.0
    for n_d in (0, 40, 320):
        sp, en = eng.rir_split(h, n_d)
        sp, en = sp.numpy(), en.numpy()
        want = split_def(h, n_d)
        assert sp.dtype == np.int32 and np.array_equal(sp, want), (n_d, sp, want)
        if n_d == 0:
            assert np.array_equal(want, [0, Lh - 1, 77, 50, 130, 257, 0])
        worst = max(worst, _db_close(en, tap_energies_def(h, want), TOL_DRR))
        for i in (3, 5):                                                                       # the NaN row's neighbours, alone
            sp1, en1 = eng.rir_split(h[i:i + 1].copy(), n_d)
            assert sp1.numpy()[0] == sp[i] and np.array_equal(en1.numpy()[0], en[i])
        assert np.isnan(en[4]).sum() == (2 if n_d == 40 else 1) and np.all(np.isfinite(np.delete(en, 4, axis=0)))
    print(f'levels rir_split energies against float64 NumPy: worst |diff| = {worst:.3g} dB (bar {TOL_DRR:g})')
    sp, en = eng.rir_split(h, 40)
    assert sp.numpy()[1] == Lh and en.numpy()[1, 1] == 0.0                                     # an empty tail: an exact 0
    sp, en = eng.rir_split(h.reshape(7, 1, Lh), 0)                                             # leading axes are kept
    assert sp.shape == (7, 1) and en.shape == (7, 1, 2) and sp.numpy()[0, 0] == 0 and en.numpy()[0, 0, 0] == 0.0
    drr, _ = dm.reverb_ratios(np.ones((7, 4), np.float32), h.reshape(7, 1, Lh), reverb_start=2.5, fs=FS)
    assert drr[1, 0] == np.inf and np.isnan(drr[4, 0]) and np.all(np.isfinite(drr[[0, 2, 3, 5, 6], 0]))


def check_nan_containment():
    """A NaN in one dry signal or in one response reaches only its own rows: every other row keeps its bits."""
    x, rir, rs, kinds, drr, srr = golden_shape(0)
    eng = _eng()
    split, _ = device_splits(eng, rir, rs)
    clean = eng.reverb_energies(x, rir, split).numpy()
    xb = x.copy()
    xb[2, 700] = np.nan
    got = eng.reverb_energies(xb, rir, split).numpy()
    assert np.all(np.isnan(got[2])) and np.array_equal(np.delete(got, 2, axis=0), np.delete(clean, 2, axis=0))
    rb = rir.copy()
    rb[3, 1, 5] = np.nan
    got = eng.reverb_energies(x, rb, split).numpy()
    assert np.isnan(got[3, 1]).any()
    got[3, 1], ref = 0.0, clean.copy()
    ref[3, 1] = 0.0
    assert np.array_equal(got, ref)
    sp, en = eng.rir_split(rb, 40)
    assert np.array_equal(np.isnan(en.numpy()).any(axis=-1), np.arange(15).reshape(5, 3) == 10)


def check_surface():
    """The refusals of both entry points with a sentinel-filled output that stays untouched; a split outside [0, rir_len] is clamped;
    device tensors and NumPy arrays give the same bits; the limit is the header's."""
    import torch
    from disco_amd import _lib
    from disco_amd import metrics as dm
    x, rir, rs, kinds, drr, srr = golden_shape(0)
    n_sig, n_ch, Lh = rir.shape
    Ld = x.shape[1]
    eng = _eng()
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'disco_hip.h')).read()
    assert f'#define DISCO_REVERB_MAX_RIR {_lib.REVERB_MAX_RIR}\n' in hdr and _lib.REVERB_MAX_RIR == 8192
    px, kx = eng.to_device(x, np.float32)
    pr, kr = eng.to_device(rir, np.float32)
    split, _ = device_splits(eng, rir, rs)
    psp, ksp = eng.to_device(split, np.int32)
    sent_e, sent_s = np.full((n_sig, n_ch, 2), -7.25), np.full((n_sig, n_ch), -3, np.int32)
    pe, ke = eng.to_device(sent_e, np.float64)
    pso, kso = eng.to_device(sent_s, np.int32)
    E_ARG, E_UNS = _lib.E_ARG, _lib.E_UNSUPPORTED

    def split_call(pr=pr, n=n_sig * n_ch, Lh=Lh, n_d=40, pso=pso, pe=pe):
        return eng.lib.disco_rir_split(eng.ctx, pr, n, Lh, n_d, pso, pe, eng.stream)

    def energy_call(px=px, pr=pr, psp=psp, n_sig=n_sig, n_ch=n_ch, Ld=Ld, Lh=Lh, pe=pe):
        return eng.lib.disco_reverb_energies(eng.ctx, px, pr, psp, n_sig, n_ch, Ld, Lh, pe, eng.stream)

    for fn, who, cases in ((split_call, 'disco_rir_split: ', ((dict(pr=None), E_ARG), (dict(pso=None), E_ARG), (dict(pe=None), E_ARG), (dict(n=-1), E_ARG),
                                                              (dict(Lh=0), E_ARG), (dict(n_d=-1), E_ARG), (dict(Lh=_lib.REVERB_MAX_RIR + 1), E_UNS))),
                           (energy_call, 'disco_reverb_energies: ', ((dict(px=None), E_ARG), (dict(pr=None), E_ARG), (dict(psp=None), E_ARG), (dict(pe=None), E_ARG),
                                                                    (dict(n_sig=-1), E_ARG), (dict(n_ch=0), E_ARG), (dict(Ld=0), E_ARG), (dict(Lh=0), E_ARG),
                                                                    (dict(Lh=_lib.REVERB_MAX_RIR + 1), E_UNS)))):
        for kw, code in cases:
            assert fn(**kw) == code, (who, kw)
            assert eng.lib.disco_last_error(eng.ctx).decode().startswith(who)
            eng.sync()
            assert np.array_equal(ke.numpy(), sent_e) and np.array_equal(kso.numpy(), sent_s), (who, kw)
    assert split_call(n=0) == 0 and energy_call(n_sig=0) == 0
    eng.sync()
    assert np.array_equal(ke.numpy(), sent_e) and np.array_equal(kso.numpy(), sent_s)
    with pytest.raises(ValueError):
        dm.reverb_ratios(x, rir[:-1])
    # a split from device memory is clamped into [0, rir_len]
    wild = split.copy()
    wild[0, 0], wild[1, 1] = -5, Lh + 7
    tame = wild.copy()
    tame[0, 0], tame[1, 1] = 0, Lh
    a, b = eng.reverb_energies(x, rir, wild).numpy(), eng.reverb_energies(x, rir, tame).numpy()
    assert np.array_equal(a, b) and a[0, 0, 0] == 0.0 and a[1, 1, 1] == 0.0 and a[0, 0, 1] > 0 and a[1, 1, 0] > 0
    # device-resident inputs: the same bits
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    want = dm.reverb_ratios(x, rir, reverb_start=2.5, fs=FS)
    got = dm.reverb_ratios(t(x), t(rir), reverb_start=2.5, fs=FS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = dm.reverb_ratios(eng.to_device(x, np.float32)[1], t(rir), reverb_start=2.5, fs=FS)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def check_reverb_at_mics():
    """dataset_utils.rooms.reverb_at_mics on source-major arrays shaped like simulate_rooms' `rirs`: both sources in one call each of the
    two entry points, equal to metrics.reverb_ratios per source; (R, Ld) inputs and the list form likewise."""
    from disco_amd import metrics as dm
    from disco_amd.dataset_utils import rooms
    x, rir, rs, kinds, drr, srr = golden_shape(0)
    S, R, n_mic = 2, 2, 3
    dry = np.stack([x[:R], x[R:2 * R]])
    rirs = np.stack([rir[:R], rir[R:2 * R]])
    out = rooms.reverb_at_mics(dry, rirs)
    assert sorted(out) == ['drr', 'split', 'srr'] and all(isinstance(v, np.ndarray) and v.shape == (S, R, n_mic) for v in out.values())
    assert out['split'].dtype == np.int32 and np.array_equal(out['split'], split_def(rirs, 320))
    for s in range(S):
        d, r = dm.reverb_ratios(dry[s], rirs[s])
        assert np.array_equal(out['drr'][s], d) and np.array_equal(out['srr'][s], r)
        one = rooms.reverb_at_mics(dry[s], rirs[s], reverb_start=20, fs=FS)
        assert one['drr'].shape == (R, n_mic) and np.array_equal(one['srr'], r) and np.array_equal(one['split'], out['split'][s])
    eng = _eng()
    lst = rooms.reverb_at_mics([dry[0], eng.to_device(dry[1], np.float32)[1]], eng.to_device(rirs, np.float32)[1])
    assert all(np.array_equal(lst[k], out[k]) for k in out)
    short = rooms.reverb_at_mics(dry, rirs, reverb_start=2.5)
    assert np.array_equal(short['split'], split_def(rirs, 40)) and not np.array_equal(short['drr'], out['drr'])
    with pytest.raises(ValueError):
        rooms.reverb_at_mics(dry, rirs[0])
