"""Checks of the per-signal spans of the metric kernels (csrc/k_metrics.h, csrc/k_bss.h: disco_pair_stats_spans, disco_band_stats_spans,
disco_lag_corr_spans, disco_bss_eval_spans, disco_bss_estimates), of `stop` arrays in disco_amd.metrics and of
results_io.batch_results: a batch of rooms of different clip lengths is scored in one call, every signal as if it ran alone.

Shared by tests/test_gpu_metric_spans.py (real MI355X, `-m gpu`) and tests/test_metric_spans_emulated.py (the same kernel sources under
the hipemu CPU emulator).  The package's own engine is used (the emulated tier binds it to the emulator).

In every check the samples at and beyond a signal's stop hold NaN (and so do those before `start` where the kernel takes a `start`):
nothing outside a span may be read, and zero padding gives the kernel under test no help.  The yardstick of a row is the existing
scalar-stop call on that signal alone, bit for bit (np.array_equal); what that call computes is pinned elsewhere (mask_metric_checks,
bss_checks, stoi_checks), and the figures are checked once more here against the oracles on the sliced signals.

Tolerances that are not bit equality:
  band variances against oracle/metrics_oracle.band_levels (scipy.signal.lfilter in float64 on the sliced signal): the bar of the
    existing band check (mask_metric_checks E): per band, BAND_FACTOR = 4 x SciPy's own relative distance from a long-double run of the
    recurrence (floor 1e-13) bounds the kernel's sums against that run; against SciPy itself its own distance comes on top (triangle
    inequality), and the variance s2 / c - (s1 / c)^2 inherits  d(s2) / c + 2 |s1| d(s1) / c^2 + (d(s1) / c)^2.
  BSS figures against the dense oracle of bss_checks: its TOL_DB.
  the room through the path (GPU file only): see check_through_the_path."""
import pickle
import warnings

import numpy as np
import scipy.signal

import bss_checks as bc
import mask_metric_checks as mmc
import stoi_checks as sc
from oracle import metrics_oracle as meo

NAN = np.float32(np.nan)


def _eng():
    from disco_amd import metrics as dm
    return dm._engine()


def nan_outside(x, start, stops):
    """copy of x (n, L) with NaN before `start` and at and beyond stops[i]"""
    x = np.array(x, dtype=np.float32)
    x[:, :start] = NAN
    for i, e in enumerate(stops):
        x[i, int(e):] = NAN
    return x


# ---- disco_pair_stats_spans ------------------------------------------------------------------------------------------------------------
def check_pair_stats(L=1000, start=100):
    stops = np.array([100, 101, 356, 357, 1000])        # empty, one sample, one full stride of 256 threads, one past it, len
    rng = np.random.default_rng(41)
    a = rng.standard_normal((len(stops), L)).astype(np.float32)
    b = rng.standard_normal((len(stops), L)).astype(np.float32)
    a[:, 150:170] = 0
    b[:, 300:420] = 0
    a, b = nan_outside(a, start, stops), nan_outside(b, start, stops)
    eng = _eng()
    for other in (b, a):
        st = eng.pair_stats(a, a if other is a else other, start, stops).numpy()
        assert st.shape == (len(stops), 8) and np.isfinite(st).all(), st
        for i, e in enumerate(stops):
            ai, oi = a[i:i + 1], other[i:i + 1]
            alone = eng.pair_stats(ai, ai if other is a else oi, start, int(e)).numpy()[0]
            assert np.array_equal(st[i], alone), (i, e, st[i], alone)
            assert st[i, 7] == e - start, (i, st[i, 7])
        assert not st[0, :7].any(), st[0]
    # NULL array = len for every signal; stops beyond [start, len] are clamped by the library
    full = np.nan_to_num(a)
    assert np.array_equal(eng.pair_stats(full, full, start, np.full(len(stops), L)).numpy(), eng.pair_stats(full, full, start).numpy())


# ---- disco_band_stats_spans ------------------------------------------------------------------------------------------------------------
# the two tables of fw_snr in full: all 18 wide-band centres (160 Hz - 8 kHz, valid from fs = 18 kHz: 14 signals per workgroup) and all 14
# narrow-band ones (200 Hz - 4 kHz, the table of fs / 2 <= 4500 Hz: 18 signals per workgroup)
BANK_FS = {'wide18': 20000, 'narrow14': 9000}


def span_bank(bank):
    fs = BANK_FS[bank]
    F = meo.band_importance(fs)[0]
    assert len(F) == int(bank[-2:])
    return meo.third_octave_filterbank(F, fs, order=4) + (np.asarray(F, float),)


def band_span_case(bank, L=775, start=5):
    """2 spb + 3 signals (two full workgroups and a partial one; 31 of them at 18 bands); within each workgroup the stops cycle through
    start (empty), one inside the first tile, the two tile edges start + 256 and start + 512, and len."""
    b, a, fc = span_bank(bank)
    spb = mmc.spb_of(b.shape[0])
    n_sig = 2 * spb + 3
    cyc = np.array([start, start + 100, start + 256, start + 512, L])
    stops = cyc[(np.arange(n_sig) % spb) % len(cyc)]
    rng = np.random.default_rng(43 + b.shape[0])
    x = rng.standard_normal((n_sig, L)).astype(np.float32)
    gate = (rng.random((n_sig, L)) < 0.6).astype(np.float32)
    return b, a, fc, stops, x, gate


def check_band_stats(bank, gated, L=775, start=5):
    b, a, fc, stops, x, gate = band_span_case(bank, L, start)
    n_sig, nb = x.shape[0], b.shape[0]
    assert n_sig >= 31 and n_sig == 2 * mmc.spb_of(nb) + 3
    xn, gn = nan_outside(x, start, stops), nan_outside(gate, start, stops)
    eng = _eng()
    st = eng.band_stats(xn, b, a, start, stops, gate=gn if gated else None).numpy()
    assert st.shape == (n_sig, nb, 3) and np.isfinite(st).all()
    for i, e in enumerate(stops):
        alone = eng.band_stats(xn[i:i + 1], b, a, start, int(e), gate=gn[i:i + 1] if gated else None).numpy()[0]
        assert np.array_equal(st[i], alone), (bank, gated, i, e)
    # the sums against the long-double recurrence at the bar of the existing band check, the variances against the oracle on the slice
    worst = 0.0
    groups = {}
    for e in np.unique(stops):
        rows = np.flatnonzero(stops == e)
        if e == start:
            assert not st[rows].any(), ('an empty span scores nothing', bank, gated)
            continue
        xs, gs = x[rows, start:e], (gate[rows, start:e] if gated else None)
        yl = mmc.lfilter_ld(b, a, xs)
        ysp = np.stack([scipy.signal.lfilter(b[j], a[j], xs.astype(np.float64), axis=-1) for j in range(nb)], axis=1)
        s1, s2, sabs = mmc._band_sums(yl, gs)
        p1, p2, _ = mmc._band_sums(ysp.astype(np.longdouble), gs)
        _, _, l1 = mmc._band_sums(ysp.astype(np.longdouble) - yl, gs)
        groups[e] = dict(rows=rows, s1=s1, s2=s2, sabs=sabs, p1=p1, p2=p2, d1=(l1 / sabs).astype(np.float64),
                         d2=(np.abs(p2 - s2) / s2).astype(np.float64), cnt=(gs.sum(-1)[:, None] if gated else np.full((len(rows), 1), float(e - start))))
    D1 = mmc._pooled(np.max([g['d1'].max(0) for g in groups.values()], axis=0), fc)          # SciPy's distance, worst signal per band
    D2 = mmc._pooled(np.max([g['d2'].max(0) for g in groups.values()], axis=0), fc)
    for e, g in groups.items():
        rows, c = g['rows'], g['cnt']
        assert np.array_equal(st[rows, :, 0], np.broadcast_to(c, (len(rows), nb))), (bank, gated, e, 'counts')
        bar1 = np.maximum(mmc.BAND_FACTOR * D1, mmc.BAND_FLOOR)[None] * g['sabs'].astype(np.float64)
        bar2 = np.maximum(mmc.BAND_FACTOR * D2, mmc.BAND_FLOOR)[None] * g['s2'].astype(np.float64)
        d1 = np.abs(st[rows, :, 1] - g['s1']).astype(np.float64)
        d2 = np.abs(st[rows, :, 2] - g['s2']).astype(np.float64)
        assert np.all(d1 <= bar1) and np.all(d2 <= bar2), (bank, gated, e, float((d1 / bar1).max()), float((d2 / bar2).max()))
        # variance of the scored samples against the oracle: the kernel's bar plus SciPy's own distance from the long-double run
        t1 = bar1 + np.maximum(D1, mmc.BAND_FLOOR)[None] * g['sabs'].astype(np.float64)
        t2 = bar2 + np.maximum(D2, mmc.BAND_FLOOR)[None] * g['s2'].astype(np.float64)
        for q, i in enumerate(rows):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                want = meo.band_levels(x[i, start:e], b, a, gate[i, start:e] if gated else None)
            cq = c[q, 0]
            if cq == 0:
                continue
            got = st[i, :, 2] / cq - (st[i, :, 1] / cq) ** 2
            tol = t2[q] / cq + 2 * np.abs(g['p1'][q].astype(np.float64)) * t1[q] / cq ** 2 + (t1[q] / cq) ** 2 + 1e-12 * np.abs(want)
            err = np.abs(got - want)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (bank, gated, i, e, float((err / tol).max()))
    print(f'band_stats spans bank {bank} gated {gated}: {n_sig} signals, worst variance error / bar = {worst:.3g}')


# ---- disco_lag_corr_spans --------------------------------------------------------------------------------------------------------------
def check_lag_corr(L=35116, start=700):
    """len - start = 2 chunks of 16384 + 1648: a third chunk of one pass that is only a tail"""
    stops = np.array([start, start + 1, start + 2048, start + 16384, start + 16385, L])
    rng = np.random.default_rng(47)
    a = nan_outside(rng.standard_normal((len(stops), L)), start, stops)
    b = nan_outside(rng.standard_normal((len(stops), L)), start, stops)
    eng = _eng()
    for lo, hi in ((-511, 511), (0, 15)):
        c = eng.lag_corr(a, b, lo, hi, start, stops).numpy()
        assert c.shape == (len(stops), hi - lo + 1) and np.isfinite(c).all()
        assert not c[0].any()
        for i, e in enumerate(stops):
            alone = eng.lag_corr(a[i:i + 1], b[i:i + 1], lo, hi, start, int(e)).numpy()[0]
            assert np.array_equal(c[i], alone), (lo, hi, i, e, float(np.abs(c[i] - alone).max()))
    # the figures themselves, where they are cheap: the short lag range of the pair that ends one past the chunk edge
    i, e = 4, int(stops[4])
    want = bc.lag_corr_oracle(a[i, start:e], b[i, start:e], range(0, 16))
    scale = np.linalg.norm(a[i, start:e].astype(np.float64)) * np.linalg.norm(b[i, start:e].astype(np.float64))
    assert np.abs(c[i] - want).max() / scale < 1e-14


# ---- disco_bss_estimates ---------------------------------------------------------------------------------------------------------------
def estimates_numpy(y, sh, szh, start, stops):
    """tango.py:547-549 as room_results states it: float64 differences rounded to float32 once; exact zeros outside the spans"""
    n, L = y.shape
    out = np.zeros((n, 3, 2, L), np.float32)
    for i, e in enumerate(stops):
        sl = slice(start, int(e))
        y64, sh64, szh64 = (v[i, sl].astype(np.float64) for v in (y, sh, szh))
        out[i, 0, 0, sl], out[i, 0, 1, sl] = sh[i, sl], (y64 - sh64).astype(np.float32)
        out[i, 1, 0, sl], out[i, 1, 1, sl] = szh[i, sl], (y64 - szh64).astype(np.float32)
        out[i, 2, 0, sl], out[i, 2, 1, sl] = y[i, sl], (y64 - sh64).astype(np.float32)
    return out


def check_bss_estimates(L=700, start=50):
    stops = np.array([50, 51, 700])
    rng = np.random.default_rng(53)
    y, sh, szh = (nan_outside(rng.standard_normal((3, L)) * 10.0 ** rng.uniform(-3, 3, (3, L)), start, stops) for _ in range(3))
    eng = _eng()
    got = eng.bss_estimates(y, sh, szh, start, stops).numpy()
    want = estimates_numpy(y, sh, szh, start, stops)
    assert got.shape == (3, 3, 2, L) and np.array_equal(got, want)
    assert not got[0].any() and not got[:, :, :, :start].any() and not got[1, :, :, 51:].any()
    # a scalar stop and None
    clean = np.nan_to_num(y), np.nan_to_num(sh), np.nan_to_num(szh)
    assert np.array_equal(eng.bss_estimates(*clean, 0, None).numpy(), estimates_numpy(*clean, 0, [L] * 3))
    assert np.array_equal(eng.bss_estimates(*clean, 7, 333).numpy(), estimates_numpy(*clean, 7, [333] * 3))


# ---- disco_bss_eval_spans --------------------------------------------------------------------------------------------------------------
def check_bss_eval_spans(L=20000, start=700, flen=64):
    """17085 = start + 16385: one sample past the first chunk.  Set 3 has an empty span: an all-zero reference."""
    from disco_amd import metrics as dm
    stops = np.array([L, 17085, 9000, start])
    kinds = ('white', 'fir', 'butter4', 'white')
    rng = np.random.default_rng(59)
    refs = np.empty((4, 2, L), np.float32)
    ests = np.empty((4, 3, 2, L), np.float32)
    for i, kind in enumerate(kinds):
        r, e = bc.make_case(kind, L, 2, seed=20 + i)
        refs[i] = r
        ests[i, 0] = e
        ests[i, 1] = e + (0.05 * rng.standard_normal(e.shape)).astype(np.float32)
        ests[i, 2] = 0.5 * e[::-1] + (0.02 * rng.standard_normal(e.shape)).astype(np.float32)
    rn = nan_outside(refs.reshape(8, L), start, np.repeat(stops, 2)).reshape(4, 2, L)
    en_ = nan_outside(ests.reshape(24, L), start, np.repeat(stops, 6)).reshape(4, 3, 2, L)
    eng = _eng()
    en, status = eng.bss_eval(rn, en_, start, stops, flen)
    assert en.shape == (4, 3, 2, 4) and status.shape == (4,)
    assert status[3] != 0 and np.isnan(en[3, ..., :3]).all() and not status[:3].any() and np.isfinite(en[:3]).all(), (status, en[3])
    worst = 0.0
    for i in range(3):
        sl = slice(start, int(stops[i]))
        r1, e1 = np.ascontiguousarray(refs[i:i + 1, :, sl]), np.ascontiguousarray(ests[i:i + 1, :, :, sl])
        alone, st1 = eng.bss_eval(r1, e1, flen=flen)
        assert st1[0] == 0 and np.array_equal(en[i], alone[0]), (i, float(np.abs(en[i] - alone[0]).max()))
        sdr, sir, sar = dm._figures(en[i])
        for k in range(3):
            for j in range(2):
                o = bc.dense_oracle(r1[0], e1[0, k, j], j, flen)
                for g, w in zip((sdr[k, j], sir[k, j], sar[k, j]), o):
                    assert np.isfinite(g) and w <= 40.0, (i, k, j, g, w)
                    worst = max(worst, abs(g - w))
    print(f'bss_eval spans: worst |err| vs the dense oracle = {worst:.3g} dB')
    assert worst < bc.TOL_DB, worst
    # chunked over sets (one set per call), the stops walk along with the sets
    en2, st2 = eng.bss_eval(rn, en_, start, stops, flen, budget_bytes=1)
    assert np.array_equal(en2, en, equal_nan=True) and np.array_equal(st2, status)


# ---- disco_amd.metrics with an array `stop` ----------------------------------------------------------------------------------------------
def check_metrics_array_stop(fs=16000, L=3000, start=100, flen=16):
    import torch
    from disco_amd import metrics as dm
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    stops = np.array([[3000, 2049], [1500, 613], [2800, 357]])
    rng = np.random.default_rng(61)
    mk = lambda scale: nan_outside((scale * rng.standard_normal((6, L))), 0, stops.reshape(-1)).reshape(3, 2, L)
    s, n = mk(0.5), mk(0.2)
    so_ = nan_outside((np.nan_to_num(s) + 0.1 * rng.standard_normal((3, 2, L))).reshape(6, L), 0, stops.reshape(-1)).reshape(3, 2, L)
    refs = np.stack([s, n], 2)                                                             # (3, 2, nsrc, L)
    est = np.stack([so_, nan_outside((np.nan_to_num(n) + 0.05 * rng.standard_normal((3, 2, L))).reshape(6, L), 0, stops.reshape(-1)).reshape(3, 2, L)], 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    calls = {
        'snr': lambda f, sel, e: f.snr(sel(s), sel(n), start=start, stop=e),
        'delta_snr': lambda f, sel, e: f.delta_snr(sel(so_), sel(n), sel(s), sel(n), start=start, stop=e),
        'sd': lambda f, sel, e: f.sd(sel(so_), sel(s), start=start, stop=e),
        'si_sdr': lambda f, sel, e: f.si_sdr(sel(s), sel(so_), start=start, stop=e),
        'si_bss': lambda f, sel, e: np.stack(f.si_bss(sel(so_), [sel(s), sel(n)], 0, start=start, stop=e)),
        'fw_snr': lambda f, sel, e: f.fw_snr(sel(s), sel(n), fs, start=start, stop=e)[1],
        'fw_sd': lambda f, sel, e: f.fw_sd(sel(so_), sel(s), fs, start=start, stop=e)[1],
        'bss_eval_sources': lambda f, sel, e: np.stack(f.bss_eval_sources(sel(refs), sel(est), compute_permutation=False, start=start, stop=e, flen=flen)[:3]),
    }
    for name, call in calls.items():
        batch = np.asarray(call(dm, lambda a: a, stops), np.float64)
        assert np.isfinite(batch).all(), (name, batch)
        for r in range(3):
            for k in range(2):
                one = np.asarray(call(dm, lambda a: a[r, k], int(stops[r, k])), np.float64)
                got = batch[..., r, k] if name == 'si_bss' else batch[:, r, k] if name == 'bss_eval_sources' else batch[r, k]
                assert np.array_equal(np.squeeze(got), np.squeeze(one)), (name, r, k, got, one)
        resident = np.asarray(call(dm, t, stops), np.float64)
        assert np.array_equal(resident, batch), (name, 'device-resident input against NumPy input')
    # stops broadcast over the leading axes, as in metrics.stoi
    per_room = np.array([[2049], [613], [357]])
    assert np.array_equal(dm.snr(s, n, start=start, stop=per_room), dm.snr(s, n, start=start, stop=np.repeat(per_room, 2, axis=1)))


# ---- results_io.batch_results -------------------------------------------------------------------------------------------------------------
ROOM_KEYS = ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')
TIME_KEYS = ('y_in', 'sh_t', 'szh_t')
LENGTHS = (32000, 28037, 24000)


def span_rooms(lengths=LENGTHS, K=2, fs=16000):
    """R rooms shaped like stoi_checks.stoi_room (speech-like target, so that STOI is meaningful), the dry sources with a white floor so
    that the Gram matrices of BSS-eval are well conditioned at 512 taps; every array holds NaN at and beyond its room's length.
    -> batch {name: (R, K, L) or (R, L)}, rooms [ {name: (K, L_r) or (L_r,)} ]"""
    L = max(lengths)
    rooms = []
    for r, Lr in enumerate(lengths):
        rng = np.random.default_rng(700 + r)
        g = sc.stoi_room(K=K, fs=fs, L=Lr, seed=5 + r)
        s_dry = g['s_dry'].astype(np.float64) + 0.01 * rng.standard_normal(Lr)
        n_dry = g['n_dry'].astype(np.float64)
        s_in = np.stack([scipy.signal.lfilter(np.r_[np.zeros(3 + 2 * k), 0.8, 0.3 * rng.standard_normal(40) * np.exp(-np.arange(40) / 12)], [1.0], s_dry) for k in range(K)])
        n_in = np.stack([scipy.signal.lfilter(np.r_[0.7, 0.2 * rng.standard_normal(30)], [1.0], n_dry) for k in range(K)])
        sf_t, nf_t = 0.9 * s_in + 0.002 * rng.standard_normal((K, Lr)), 0.3 * n_in
        szf_t, nzf_t = 0.8 * s_in + 0.004 * rng.standard_normal((K, Lr)), 0.6 * n_in
        d = dict(s_in=s_in, n_in=n_in, sf_t=sf_t, nf_t=nf_t, szf_t=szf_t, nzf_t=nzf_t, s_dry=s_dry, n_dry=n_dry, y_in=s_in + n_in,
                 sh_t=sf_t + nf_t, szh_t=szf_t + nzf_t)
        rooms.append({k: np.asarray(v, np.float32) for k, v in d.items()})
    batch = {}
    for name in rooms[0]:
        a = np.full((len(lengths),) + rooms[0][name].shape[:-1] + (L,), NAN, np.float32)
        for r, g in enumerate(rooms):
            a[r, ..., :g[name].shape[-1]] = g[name]
        batch[name] = a
    return batch, rooms


def _room_alone(g, snrs, bss_flen, fs, cut=None):
    from disco_amd.speech_enhancement import results_io as rio
    c = (lambda a: a) if cut is None else (lambda a: np.ascontiguousarray(a[..., :cut]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return rio.room_results(*(c(g[k]) for k in ROOM_KEYS), rnd_snrs=snrs, s_dry=c(g['s_dry']), n_dry=c(g['n_dry']), fs=fs,
                                **{k: c(g[k]) for k in TIME_KEYS}, bss_flen=bss_flen, stoi=True)


def _assert_rows(res, resz, r, alone, what):
    from disco_amd.speech_enhancement import results_io as rio
    assert tuple(res) == rio.RESULT_KEYS_TANGO and tuple(resz) == rio.RESULT_KEYS_MWF
    for got, want in ((res, alone[0]), (resz, alone[1])):
        for key in got:
            np.testing.assert_array_equal(np.asarray(got[key])[r], np.asarray(want[key]), err_msg=f'{what}: key {key}, room {r}')


def check_batch_results(bss_flen, tmp_path, fs=16000):
    import torch
    from disco_amd.speech_enhancement import results_io as rio
    batch, rooms = span_rooms()
    R, K = batch['s_in'].shape[:2]
    snrs = np.array([[3.0, 1.0], [0.5, -2.0], [6.0, 4.0]])
    kw = dict(s_dry=batch['s_dry'], n_dry=batch['n_dry'], fs=fs, bss_flen=bss_flen, stoi=True, **{k: batch[k] for k in TIME_KEYS})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res, resz = rio.batch_results(*(batch[k] for k in ROOM_KEYS), snrs, lengths=np.array(LENGTHS), **kw)
    alone = [_room_alone(rooms[r], snrs[r], bss_flen, fs) for r in range(R)]
    for r in range(R):
        _assert_rows(res, resz, r, alone[r], 'mixed lengths')
    for d in (res, resz):
        for key, v in d.items():
            assert np.shape(v) == (R, K), (key, np.shape(v))
            assert np.all(np.isfinite(v)) or key == 'snr_in_raw', (key, v)
    assert res['snr_in_raw'] is snrs
    print('batch_results, mixed lengths: sdr_cnv', res['sdr_cnv'].tolist(), 'snr_out', res['snr_out'].tolist(), 'delta_stoi_cnv', res['delta_stoi_cnv'].tolist())
    # device-resident tensors are read in place: the same bits
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    t = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        rt, rzt = rio.batch_results(*(t[k] for k in ROOM_KEYS), snrs, s_dry=t['s_dry'], n_dry=t['n_dry'], fs=fs, bss_flen=bss_flen, stoi=True,
                                    lengths=list(LENGTHS), **{k: t[k] for k in TIME_KEYS})
    for a, b in ((res, rt), (resz, rzt)):
        for key in a:
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=f'device-resident input: key {key}')
    # lengths=None on a uniform batch: the common last axis, as room_results takes it (rooms 2 and 0 cut to the shortest clip)
    cut = min(LENGTHS)
    uni = {k: np.ascontiguousarray(v[[2, 0], ..., :cut]) for k, v in batch.items()}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        ru, rzu = rio.batch_results(*(uni[k] for k in ROOM_KEYS), snrs[[2, 0]], s_dry=uni['s_dry'], n_dry=uni['n_dry'], fs=fs, bss_flen=bss_flen,
                                    stoi=True, **{k: uni[k] for k in TIME_KEYS})
    _assert_rows(ru, rzu, 0, alone[2], 'uniform batch, lengths=None')
    _assert_rows(ru, rzu, 1, _room_alone(rooms[0], snrs[0], bss_flen, fs, cut=cut), 'uniform batch, lengths=None')
    # without the time signals / the dry sources the keys hold NaN, as in room_results
    r3, rz3 = rio.batch_results(*(batch[k] for k in ROOM_KEYS), snrs, fs=fs, lengths=LENGTHS)
    for key in rio.THIRD_PARTY_KEYS + ('snr_in_dry', 'fw_sd_dry'):
        assert all(np.all(np.isnan(d[key])) for d in (r3, rz3) if key in d), key
    np.testing.assert_array_equal(r3['snr_out'], res['snr_out'])
    # one room out of the batch, into the pickles of the reference
    one, onez = rio.results_of_room(res, resz, 1)
    _assert_rows({k: np.asarray(v)[None] for k, v in one.items()}, {k: np.asarray(v)[None] for k, v in onez.items()}, 0, alone[1], 'results_of_room')
    files = rio.write_result_pickles(str(tmp_path), 11002, 'ssn', one, onez)
    for f, d in zip(files, (one, onez)):
        back = pickle.load(open(f, 'rb'))
        assert list(back) == list(d)
        for key in d:
            np.testing.assert_array_equal(back[key], d[key])


def check_batch_zero_reference(fs=16000):
    """an all-zero reference raises ValueError naming the room and the node"""
    import pytest
    from disco_amd.speech_enhancement import results_io as rio
    L, lengths = fs + 3000, (fs + 3000, fs + 2000)
    rng = np.random.default_rng(67)
    sig = {k: nan_outside(0.1 * rng.standard_normal((4, L)), 0, np.repeat(lengths, 2)).reshape(2, 2, L) for k in ROOM_KEYS + TIME_KEYS}
    sig['s_in'][1, 1, :lengths[1]] = 0
    dry = [nan_outside(0.1 * rng.standard_normal((2, L)), 0, lengths) for _ in range(2)]
    with pytest.raises(ValueError, match='room 1, node 1: reference source 0 is all zero'), np.errstate(all='ignore'):
        rio.batch_results(*(sig[k] for k in ROOM_KEYS), [0, 0], s_dry=dry[0], n_dry=dry[1], fs=fs, bss_flen=8, lengths=lengths,
                          **{k: sig[k] for k in TIME_KEYS})
    sig['s_in'][1, 1, :lengths[1]] = 0.1 * rng.standard_normal(lengths[1]).astype(np.float32)
    dry[1][0, :lengths[0]] = 0
    with pytest.raises(ValueError, match='room 0, every node .dry sources.: reference source 1 is all zero'), np.errstate(all='ignore'):
        rio.batch_results(*(sig[k] for k in ROOM_KEYS), [0, 0], s_dry=dry[0], n_dry=dry[1], fs=fs, bss_flen=8, lengths=lengths,
                          **{k: sig[k] for k in TIME_KEYS})


# ---- through the path (GPU file only) -------------------------------------------------------------------------------------------------------
# Tolerances of a room of the mixed batch against the same room alone in an engine of its own length.  The path's own mixed-length tests
# (length_checks.check_whole_path, check_reference_outputs) hold both within tol = 1e-4 (relative l2 error per node) of the float64 oracle,
# hence within eps = 2e-4 of each other; nothing is bit-equal there, so nothing is here.  What eps does to a key:
#   level keys (fw_snr, fw_sd: importance-weighted mean over bands of a clipped level ratio in dB, weights summing to 1): a band level moves
#     by (20 / ln 10) eps_band dB, and both levels of a ratio may move.  eps_band <= eps |x| / |x_band|: at worst the whole error sits in one
#     band.  The narrowest band (160 Hz, 37 Hz wide of 8 kHz) holds 0.46 % of the energy of a white signal: |x| / |x_band| = 14.7.
#     -> 2 x 8.69 x 14.7 x 2e-4 = 0.051 dB.
#   BSS keys (10 log10 of a ratio of energies; the smaller one is a residual that is 10^(-S / 20) of the estimate in amplitude for a figure
#     of S dB): the residual moves by eps 10^(S / 20) relative to itself, the larger energy by eps: (20 / ln 10) eps (1 + 10^(S / 20)) dB, S
#     the figure of the room alone; each estimate holds two path outputs (y - sh): twice that.
#   STOI keys (a difference of two correlation coefficients of band envelopes): a band envelope moves by eps_band relative to itself, a
#     correlation coefficient of unit vectors by at most twice that, per STOI value; two values per key: 4 x 14.7 x 2e-4 = 0.012.
EPS_PATH = 2e-4
TOL_LEVEL_DB = 2 * (20 / np.log(10)) * 14.7 * EPS_PATH
TOL_STOI = 4 * 14.7 * EPS_PATH


def tol_bss_db(figure_db):
    return 2 * (20 / np.log(10)) * EPS_PATH * (1 + 10 ** (np.abs(figure_db) / 20))


def check_through_the_path(make_engine, lengths=LENGTHS, K=2, M=2, fs=16000, bss_flen=512):
    """Engine.set_lengths -> tango_reference -> istft -> batch_results, all device-resident, against room_results of each room run alone
    in an engine of its own length."""
    import torch
    from disco_amd import synth
    from disco_amd.speech_enhancement import results_io as rio
    R, L = len(lengths), max(lengths)
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    rng = np.random.default_rng(71)
    s_dry, n_dry = (0.3 * rng.standard_normal((R, L))).astype(np.float32), (0.3 * rng.standard_normal((R, L))).astype(np.float32)
    for r in range(R):
        s_dry[r, 40:] += 0.5 * s[r, 0, 0, :-40]                            # the dry sources are not unrelated to what the nodes hear
        n_dry[r, 25:] += 0.5 * n[r, 0, 0, :-25]
    own = [tuple(np.ascontiguousarray(a[r, ..., :lengths[r]]) for a in (y, s, n, s_dry, n_dry)) for r in range(R)]
    for a in (y, s, n, s_dry, n_dry):
        for r in range(R):
            a[r, ..., lengths[r]:] = NAN
    snrs = np.arange(R * K, dtype=np.float64).reshape(R, K)
    names = ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n')

    def enhance(eng, y_, s_, n_, to_torch):
        Rr, Lr = y_.shape[0], y_.shape[-1]
        yd, sd_, nd = (eng.to_device(a, np.float32)[1] for a in (y_, s_, n_))
        spec = eng.tango_reference(yd, sd_, nd, want=names)
        out = {}
        for nm in names:
            if to_torch:
                buf = torch.empty((Rr * K, Lr), dtype=torch.float32, device='cuda')
                eng.istft(spec[nm].reshape(Rr * K, eng.T, eng.F), out=buf)
                out[nm] = buf.reshape(Rr, K, Lr)
            else:
                out[nm] = eng.istft(spec[nm].reshape(Rr * K, eng.T, eng.F)).numpy().reshape(Rr, K, Lr)
        return out

    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    eng.set_lengths(lengths)
    t = enhance(eng, y, s, n, True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda')
    res, resz = rio.batch_results(dev(s[:, :, 0]), dev(n[:, :, 0]), t['sf'], t['nf'], t['z_s'], t['z_n'], snrs, s_dry=dev(s_dry), n_dry=dev(n_dry),
                                  fs=fs, y_in=dev(y[:, :, 0]), sh_t=t['yf'], szh_t=t['z_y'], bss_flen=bss_flen, stoi=True, lengths=np.array(lengths))
    worst = {}
    for r, Lr in enumerate(lengths):
        yr, sr, nr, sdr_, ndr = own[r]
        solo = make_engine(rooms=1, nodes=K, mics=M, length=int(Lr))
        a = enhance(solo, yr[None], sr[None], nr[None], False)
        for nm in names:                                                   # the premise: the path's own tolerance, alone against batched
            got = t[nm][r, :, :Lr].cpu().numpy()
            assert not t[nm][r, :, Lr:].cpu().numpy().any()
            e = max(float(np.linalg.norm(got[k] - a[nm][0, k]) / np.linalg.norm(a[nm][0, k])) for k in range(K))
            worst['path ' + nm] = max(worst.get('path ' + nm, 0.0), e)
            assert e < EPS_PATH, (nm, r, e)
        one, onez = rio.room_results(sr[:, 0], nr[:, 0], a['sf'][0], a['nf'][0], a['z_s'][0], a['z_n'][0], snrs[r], s_dry=sdr_, n_dry=ndr, fs=fs,
                                     y_in=yr[:, 0], sh_t=a['yf'][0], szh_t=a['z_y'][0], bss_flen=bss_flen, stoi=True)
        # the new code alone: the batch's own signals, room r cut out and scored by room_results -- bit for bit
        cutr = lambda x: np.ascontiguousarray(x[r, ..., :Lr].cpu().numpy())
        same, samez = rio.room_results(sr[:, 0], nr[:, 0], cutr(t['sf']), cutr(t['nf']), cutr(t['z_s']), cutr(t['z_n']), snrs[r], s_dry=sdr_,
                                       n_dry=ndr, fs=fs, y_in=yr[:, 0], sh_t=cutr(t['yf']), szh_t=cutr(t['z_y']), bss_flen=bss_flen, stoi=True)
        _assert_rows(res, resz, r, (same, samez), 'through the path, the batch signals scored per room')
        for got, want in ((res, one), (resz, onez)):
            for key in got:
                g, w = np.asarray(got[key])[r], np.asarray(want[key])
                if key == 'snr_in_raw':
                    assert np.array_equal(g, w)
                    continue
                assert np.isfinite(g).all() and np.isfinite(w).all(), (key, r, g, w)
                tol = TOL_STOI if 'stoi' in key else tol_bss_db(w) if key in rio.BSS_KEYS else TOL_LEVEL_DB
                d = np.abs(g - w)
                worst[key] = max(worst.get(key, 0.0), float(d.max()))
                assert np.all(d <= tol), (key, r, g, w, tol)
    print('through the path, batch_results against rooms alone: worst differences', {k: float(f'{v:.3g}') for k, v in worst.items()})
