"""Checks of the segmental SNR (disco_seg_snr, csrc/k_segsnr.h; disco_amd.metrics.seg_snr), of its keys in room_results / batch_results
and of ci_wp / bar_data, shared by tests/test_levels_emulated.py (hipemu) and tests/test_gpu_levels.py (MI355X).

The yardstick is tests/golden/levels_ref.npz: the reference's own seg_snr / ci_wp / bar_data run on float64 copies of the float32 inputs
(tests/golden/make_golden_levels.py, whose case tables are imported here).

Bars, derived and not taken from the code under test:
  TOL_SEG = 1e-9 dB   each variance is a float64 two-pass sum of at most W terms (about W 2^-53 relative), the log and the clipped mean add
                      a few ulp; 1e-9 leaves three decades.
  TOL_TABLE = 1e-15   relative, ci_wp / bar_data against the golden values (the same NumPy calls on the same numbers).
Measured (lines starting `levels `): seg_snr against the golden values, worst |diff| 6.2e-15 dB on the MI355X and under hipemu (53 cases, 11
of them NaN on both sides); ci_wp / bar_data 0.
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SEG = 1e-9
TOL_TABLE = 1e-15

_spec = importlib.util.spec_from_file_location('make_golden_levels', os.path.join(HERE, 'golden', 'make_golden_levels.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(HERE, 'golden', 'levels_ref.npz')) as z:
            _golden = {k: z[k] for k in z.files}
        s, n, vad = gen.seg_signals()                    # the fixture holds what the generator makes
        assert np.array_equal(_golden['seg_s'], s) and np.array_equal(_golden['seg_n'], n) and np.array_equal(_golden['seg_vad'], vad)
        assert np.array_equal(_golden['seg_cases'], gen.seg_cases())
    return _golden


def _eng():
    from disco_amd import metrics as dm
    return dm._engine()


def _close(got, want, tol):
    """NaN exactly where the yardstick has it, |diff| below tol elsewhere -> worst |diff|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    worst = float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0
    assert worst < tol, (worst, tol, got, want)
    return worst


def check_golden():
    """Every case of the fixture through metrics.seg_snr on the sliced 1-D signals (the reference's own call shape), and all cases of one
    window size in one batched call with start and a stop per signal."""
    from disco_amd import metrics as dm
    g = golden()
    s, n, vad, cases, ref = g['seg_s'], g['seg_n'], g['seg_vad'], g['seg_cases'], g['seg_ref']
    got = np.empty(len(cases))
    for q, (row, start, stop, w, h, v) in enumerate(cases):
        gv = None if v == gen.VAD_NONE else vad[v, start:stop]
        got[q] = dm.seg_snr(s[row, start:stop], n[row, start:stop], int(w), int(h), vad=gv)
        assert isinstance(got[q], float)
    worst = _close(got, ref, TOL_SEG)
    print(f'levels seg_snr golden: {len(cases)} cases ({int(np.isnan(ref).sum())} NaN), worst |diff| = {worst:.3g} dB (bar {TOL_SEG:g})')
    assert np.isnan(ref).sum() >= 5 and np.sum(ref == 0.0) >= 3                 # no whole window / zero weights; the floor's 0 dB
    # the same cases batched: one call per (window, start, VAD kind), a stop per signal -- equal to the 1-D calls bit for bit
    keys = sorted({(int(w), int(h), int(start), int(v)) for _, start, _, w, h, v in cases})
    for w, h, start, v in keys:
        idx = [q for q, c in enumerate(cases) if (int(c[3]), int(c[4]), int(c[1]), int(c[5])) == (w, h, start, v)]
        rows, stops = cases[idx, 0], cases[idx, 2]
        gv = None if v == gen.VAD_NONE else np.broadcast_to(vad[v], (len(idx), s.shape[1]))
        batched = dm.seg_snr(s[rows], n[rows], w, h, vad=gv, start=start, stop=stops)
        assert batched.shape == (len(idx),) and np.array_equal(batched, got[idx], equal_nan=True), (w, h, start, v)


def check_clip_and_floor_counts():
    """The raw sums of the entry point: N_w of every span length, the clip count, the floor's exact 0 dB where both signals are zero."""
    g = golden()
    s, n = g['seg_s'], g['seg_n']
    eng = _eng()
    for w, h in gen.SEG_WINDOWS:
        lens = np.array([w - 1, w, w + h - 1, w + h, 6000])
        st = eng.seg_snr(s[np.zeros(5, int)], n[np.zeros(5, int)], w, h, stop=lens).numpy()
        assert np.array_equal(st[:, 2], np.where(lens >= w, (lens - w) // h + 1, 0)), (w, h, st[:, 2])
        assert np.array_equal(st[:, 1], st[:, 2]) and st[0, 0] == 0.0 and np.all(st[:, 3] <= st[:, 2])
    st = eng.seg_snr(s[1:2, 3584:4352].copy(), n[1:2, 3584:4352].copy(), 256, 128).numpy()     # both exactly zero: eps / eps
    assert st[0, 0] == 0.0 and st[0, 2] == 5 and st[0, 3] == 0
    st = eng.seg_snr(s[1:2, 512:1280].copy(), n[1:2, 512:1280].copy(), 256, 128).numpy()       # s exactly zero: the lower bound
    assert st[0, 0] == -15.0 * 5 and st[0, 3] == 5
    st = eng.seg_snr(s[1:2, 2048:2816].copy(), n[1:2, 2048:2816].copy(), 256, 128).numpy()     # n exactly zero: the upper bound
    assert st[0, 0] == 25.0 * 5 and st[0, 3] == 5
    st = eng.seg_snr(s[:1], n[:1], 512, 256, lo_db=-1.0, hi_db=1.0).numpy()                     # other bounds reach the kernel
    assert abs(st[0, 0]) <= st[0, 2] and st[0, 3] > 0


def check_rows_alone_and_nan():
    """start = 300 with a stop per signal: every row has the bits of the row scored alone on its slice, whatever sits at and beyond its
    stop (NaN here); a NaN inside one row makes that row NaN and changes no bit of the others; run to run the same bits."""
    from disco_amd import metrics as dm
    g = golden()
    s, n, vad = g['seg_s'].copy(), g['seg_n'].copy(), g['seg_vad']
    stops = np.array([6300, 5321, 4000])
    gv = np.stack([vad[1], vad[0], vad[1]])
    for i, e in enumerate(stops):
        s[i, e:] = n[i, e:] = np.nan
    gv = gv.copy()
    gv[1, stops[1]:] = np.nan
    got = dm.seg_snr(s, n, 512, 256, vad=gv, start=300, stop=stops)
    assert np.all(np.isfinite(got)), got
    assert np.array_equal(got, dm.seg_snr(s, n, 512, 256, vad=gv, start=300, stop=stops))
    for i, e in enumerate(stops):
        alone = dm.seg_snr(s[i, 300:e], n[i, 300:e], 512, 256, vad=gv[i, 300:e])
        assert alone == got[i], (i, alone, got[i])
    assert np.array_equal(dm.seg_snr(s.reshape(3, 1, -1), n.reshape(3, 1, -1), 512, 256, vad=gv.reshape(3, 1, -1), start=300, stop=stops[:, None]),
                          got.reshape(3, 1))
    s[1, 2000] = np.nan
    hit = dm.seg_snr(s, n, 512, 256, vad=gv, start=300, stop=stops)
    assert np.isnan(hit[1]) and hit[0] == got[0] and hit[2] == got[2], (hit, got)


def check_device_resident():
    """A device tensor and a NumPy array as input give the same bits."""
    import torch
    from disco_amd import metrics as dm
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    g = golden()
    s, n, vad = g['seg_s'], g['seg_n'], g['seg_vad']
    stops = np.array([6300, 5321, 4000])
    want = dm.seg_snr(s, n, 400, 160, vad=vad, start=300, stop=stops)
    assert np.array_equal(np.isnan(want), [False, False, True])                                # the all-zero VAD row
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    assert np.array_equal(dm.seg_snr(t(s), t(n), 400, 160, vad=t(vad), start=300, stop=stops), want, equal_nan=True)
    eng = _eng()
    ds = eng.to_device(s, np.float32)[1]
    assert np.array_equal(dm.seg_snr(ds, t(n), 400, 160, vad=t(vad), start=300, stop=stops), want, equal_nan=True)
    assert np.array_equal(dm.seg_snr(t(s), t(n), 400, 160), dm.seg_snr(s, n, 400, 160))


def check_surface():
    """Unequal shapes raise ValueError; the refusals of disco_seg_snr return the documented codes and leave a sentinel-filled `out` as it
    was; the window limit is the header's, refused at limit + 1 and accepted at the limit."""
    from disco_amd import _lib
    from disco_amd import metrics as dm
    g = golden()
    s, n = g['seg_s'][:2], g['seg_n'][:2]
    with pytest.raises(ValueError, match='same shape'):
        dm.seg_snr(s[0], n[0, :-1], 512, 256)
    with pytest.raises(ValueError, match='vad'):
        dm.seg_snr(s, n, 512, 256, vad=g['seg_vad'][0])
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'disco_hip.h')).read()
    assert f'#define DISCO_SEG_SNR_MAX_WIN {_lib.SEG_SNR_MAX_WIN}\n' in hdr and _lib.SEG_SNR_MAX_WIN >= 2048
    eng = _eng()
    n_sig, L = s.shape
    ps, ks = eng.to_device(s, np.float32)
    pn, kn = eng.to_device(n, np.float32)
    sentinel = np.full((n_sig, 4), -7.25)
    po, out = eng.to_device(sentinel, np.float64)

    def call(ps=ps, pn=pn, po=po, n_sig=n_sig, start=0, w=512, h=256, lo=-15.0, hi=25.0):
        return eng.lib.disco_seg_snr(eng.ctx, ps, pn, None, n_sig, L, start, None, w, h, lo, hi, po, eng.stream)

    E_ARG, E_UNS = _lib.E_ARG, _lib.E_UNSUPPORTED
    for kw, code in ((dict(w=0), E_ARG), (dict(h=0), E_ARG), (dict(w=256, h=257), E_ARG), (dict(lo=25.0, hi=25.0), E_ARG), (dict(lo=3.0, hi=-3.0), E_ARG),
                     (dict(ps=None), E_ARG), (dict(pn=None), E_ARG), (dict(po=None), E_ARG), (dict(n_sig=-1), E_ARG), (dict(start=-1), E_ARG),
                     (dict(start=L + 1), E_ARG), (dict(w=_lib.SEG_SNR_MAX_WIN + 1), E_UNS)):
        assert call(**kw) == code, kw
        assert eng.lib.disco_last_error(eng.ctx).decode().startswith('disco_seg_snr: ')
        eng.sync()
        assert np.array_equal(out.numpy(), sentinel), kw
    assert call(n_sig=0) == 0
    eng.sync()
    assert np.array_equal(out.numpy(), sentinel)
    assert call(w=_lib.SEG_SNR_MAX_WIN, h=1000) == 0
    eng.sync()
    st = out.numpy()
    W = _lib.SEG_SNR_MAX_WIN
    v = 10 * np.log10(np.maximum(np.var(s[:, :W].astype(np.float64), axis=1), 2.220446049250313e-16) / np.var(n[:, :W].astype(np.float64), axis=1))
    assert np.all(st[:, 2] == (L - W) // 1000 + 1) and st[0, 2] >= 2
    one = eng.seg_snr(s[:, :W].copy(), n[:, :W].copy(), W, 1000).numpy()
    assert np.all(np.abs(one[:, 0] - np.clip(v, -15, 25)) < TOL_SEG), (one[:, 0], v)


def check_room_results(fs=16000):
    """room_results(seg_snr=True): the two new keys of each dictionary equal direct metrics.seg_snr calls on the scored span, to the bit;
    the default dictionaries are what they were."""
    import stoi_checks as sc
    from disco_amd import metrics as dm
    from disco_amd import sigproc_utils as su
    from disco_amd.speech_enhancement import results_io as rio
    g = sc.stoi_room(L=16000 + 6000)
    pos = [g[k] for k in ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')]
    res, resz = rio.room_results(*pos, rnd_snrs=[3.0], fs=fs, seg_snr=True)
    assert rio.SEG_SNR_KEYS == ('seg_snr_in_cnv', 'seg_snr_out')
    assert tuple(res) == rio.RESULT_KEYS_TANGO + rio.SEG_SNR_KEYS and tuple(resz) == rio.RESULT_KEYS_MWF + rio.SEG_SNR_KEYS
    cut = lambda a: np.ascontiguousarray(a[..., fs:])
    vad = su.vad_oracle_batch(cut(g['s_in']))
    assert 0 < vad.mean() < 1 or vad.mean() == 1
    want = {('res', 'seg_snr_in_cnv'): ('s_in', 'n_in'), ('res', 'seg_snr_out'): ('sf_t', 'nf_t'), ('resz', 'seg_snr_in_cnv'): ('s_in', 'n_in'),
            ('resz', 'seg_snr_out'): ('szf_t', 'nzf_t')}
    for (which, key), (a, b) in want.items():
        direct = dm.seg_snr(cut(g[a]), cut(g[b]), 512, 256, vad=vad)
        got = (res if which == 'res' else resz)[key]
        print(f'{which}[{key}] = {got}')
        assert np.all(np.isfinite(got)) and np.array_equal(got, direct), (which, key, got, direct)
    r0, rz0 = rio.room_results(*pos, rnd_snrs=[3.0], fs=fs)
    assert tuple(r0) == rio.RESULT_KEYS_TANGO and tuple(rz0) == rio.RESULT_KEYS_MWF
    for r, rr in ((res, r0), (resz, rz0)):
        for key in rr:
            assert np.array_equal(np.asarray(r[key]), np.asarray(rr[key]), equal_nan=True), key


def check_batch_results(fs=16000):
    """batch_results(seg_snr=True) on two rooms of different lengths, NaN past the shorter clip: each room's row is that room scored alone
    at its own length, to the bit; host arrays and device tensors agree; the default adds no key."""
    import stoi_checks as sc
    from disco_amd.speech_enhancement import results_io as rio
    rooms = [sc.stoi_room(L=16000 + 6000, seed=5), sc.stoi_room(L=16000 + 6000, seed=6)]
    L = rooms[0]['s_in'].shape[-1]
    lens = np.array([L, L - 1801])
    names = ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')

    def stack(nm):
        a = np.stack([g[nm] for g in rooms])
        a[1, ..., lens[1]:] = np.nan
        return a

    kw = dict(rnd_snrs=np.array([[3.0], [1.0]]), fs=fs, lengths=lens)
    res, resz = rio.batch_results(*(stack(nm) for nm in names), seg_snr=True, **kw)
    assert tuple(res) == rio.RESULT_KEYS_TANGO + rio.SEG_SNR_KEYS and tuple(resz) == rio.RESULT_KEYS_MWF + rio.SEG_SNR_KEYS
    for r, g in enumerate(rooms):
        one, onez = rio.room_results(*(g[nm][..., :lens[r]] for nm in names), rnd_snrs=[3.0], fs=fs, seg_snr=True)
        for got, want in ((res, one), (resz, onez)):
            for key in rio.SEG_SNR_KEYS:
                assert np.all(np.isfinite(got[key][r])) and np.array_equal(got[key][r], want[key]), (r, key, got[key][r], want[key])
    b0, bz0 = rio.batch_results(*(stack(nm) for nm in names), **kw)
    assert tuple(b0) == rio.RESULT_KEYS_TANGO and tuple(bz0) == rio.RESULT_KEYS_MWF
    assert all(np.array_equal(np.asarray(b0[k]), np.asarray(res[k]), equal_nan=True) for k in b0)
    import torch
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    rt, rzt = rio.batch_results(*(torch.from_numpy(stack(nm)).to(dev) for nm in names), seg_snr=True, **kw)
    for key in rio.SEG_SNR_KEYS:
        assert np.array_equal(rt[key], res[key]) and np.array_equal(rzt[key], resz[key]), key


def check_tables():
    """ci_wp and bar_data against the reference's own values, NaN pattern included.  Host NumPy: no library needed."""
    from disco_amd import metrics as dm
    from disco_amd import misc_utils as mu
    g = golden()
    worst = 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            pairs = [(dm.ci_wp(g['ci_x']), g['ci_axis0']), (dm.ci_wp(g['ci_x'], axis=1), g['ci_axis1'])]
    means, cis = mu.bar_data(g['bar_edges'], g['bar_x'], g['bar_y'])
    pairs += [(means, g['bar_means']), (cis, g['bar_cis'])]
    for got, want in pairs:
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
        ok = ~np.isnan(want)
        rel = np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))
        worst = max(worst, float(rel))
        assert rel <= TOL_TABLE, (rel, got, want)
    assert np.isnan(g['bar_means']).sum() == 1 and np.isnan(g['ci_axis0']).sum() == 1            # the empty bin, the all-NaN column
    print(f'levels ci_wp / bar_data golden: worst relative diff = {worst:.3g} (bar {TOL_TABLE:g})')
    with pytest.raises(ValueError):
        mu.bar_data(g['bar_edges'], np.array([99.0]), np.array([1.0]))
