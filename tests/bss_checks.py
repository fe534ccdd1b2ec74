"""Checks of the BSS-eval kernels (csrc/k_bss.h: disco_lag_corr, disco_bss_eval) and their Python surface
(disco_amd.metrics.bss_eval_sources, Engine.bss_eval, results_io.room_results with y_in / sh_t / szh_t).

Shared by tests/test_gpu_bss.py (real MI355X, `-m gpu`, full sizes) and tests/test_bss_emulated.py (the same kernel sources under the
hipemu CPU emulator, small sizes); tests/test_bss_cpu.py pins the two yardsticks below against each other.

mir_eval is absent, so the feature is pinned by definition (Vincent, Gribonval, Fevotte 2006), with two float64 NumPy / SciPy oracles:
  dense   the matrix of delayed, zero-padded references is formed, the estimate projected with np.linalg.lstsq on the target's columns
          and on all columns, the residual SIGNALS formed and their energies summed.  For L up to about 8000.
  gram    lag correlations (direct dot products), the block-Toeplitz Gram matrix with source j first, scipy cho_factor, forward
          substitution.  For full-length signals.
Tolerance of the kernels against an oracle: TOL_DB = 1e-6 dB on SDR, SIR and SAR for cases with cond(G) <= 1e11 and every figure
<= 40 dB: the two unrelated float64 routes agree to 1e-9 dB or better on such inputs (2e-12 at cond <= 5e6), which leaves three to
five orders for another summation order and a blocked factorisation, and is 200 x tighter than the 2e-4 dB of the float32-fed level
metrics."""
import numpy as np
import scipy.linalg
import scipy.signal

TOL_DB = 1e-6
SPECTRA = ('white', 'fir', 'butter4', 'butter8')


# ---- the oracles ---------------------------------------------------------------------------------------------------------------

def _db(num, den):
    den = max(den, 0.0)
    if den == 0:
        return np.inf
    with np.errstate(divide='ignore'):
        return 10 * np.log10(num / den)


def dense_oracle(refs, est, j, flen):
    """refs (nsrc, L), est (L,) -> (sdr, sir, sar) of `est` against source j, residuals formed as signals."""
    refs, est = np.asarray(refs, np.float64), np.asarray(est, np.float64)
    nsrc, L = refs.shape
    A = np.zeros((L + flen - 1, nsrc * flen))
    for p in range(nsrc):
        for a in range(flen):
            A[a:a + L, p * flen + a] = refs[p]
    e = np.zeros(L + flen - 1)
    e[:L] = est
    Aj = A[:, j * flen:(j + 1) * flen]
    s_target = Aj @ np.linalg.lstsq(Aj, e, rcond=None)[0]
    p_all = A @ np.linalg.lstsq(A, e, rcond=None)[0]
    e_interf, e_artif = p_all - s_target, e - p_all
    return (_db(s_target @ s_target, (e_interf + e_artif) @ (e_interf + e_artif)), _db(s_target @ s_target, e_interf @ e_interf),
            _db((s_target + e_interf) @ (s_target + e_interf), e_artif @ e_artif))


def lag_corr_oracle(a, b, lags):
    """c[t] = sum_n a[n] b[n + t] (no wrap), direct float64 dot products."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    L = len(a)
    out = np.zeros(len(lags))
    for i, t in enumerate(lags):
        if t >= 0:
            out[i] = a[:L - t] @ b[t:] if t < L else 0.0
        else:
            out[i] = a[-t:] @ b[:L + t] if -t < L else 0.0
    return out


def gram_matrix(refs, flen, order=None):
    refs = np.asarray(refs, np.float64)
    nsrc = refs.shape[0]
    order = list(range(nsrc)) if order is None else order
    c = {(p, q): lag_corr_oracle(refs[p], refs[q], range(flen)) for p in range(nsrc) for q in range(nsrc)}
    # block (p, q) entry (a, b) = c_pq[a - b]: first column c_pq[a], first row c_pq[-b] = c_qp[b]
    return np.block([[scipy.linalg.toeplitz(c[p, q], c[q, p]) for q in order] for p in order])


def gram_oracle(refs, est, j, flen):
    """The same figures from lag correlations, one Cholesky factorisation with source j first -> (sdr, sir, sar)."""
    refs, est = np.asarray(refs, np.float64), np.asarray(est, np.float64)
    nsrc = refs.shape[0]
    order = [j] + [p for p in range(nsrc) if p != j]
    G = gram_matrix(refs, flen, order)
    d = np.concatenate([lag_corr_oracle(refs[p], est, range(flen)) for p in order])
    Lc, low = scipy.linalg.cho_factor(G, lower=True)
    y = scipy.linalg.solve_triangular(Lc, d, lower=True)
    pj, pall, ee = float(y[:flen] @ y[:flen]), float(y @ y), float(est @ est)
    return _db(pj, ee - pj), _db(pj, pall - pj), _db(pall, ee - pall)


def cond_gram(refs, flen):
    return float(np.linalg.cond(gram_matrix(refs, flen)))


# ---- inputs (regenerated from fixed seeds; float32, as the kernels read them) ----------------------------------------------------

def _shaped(rng, kind, L):
    w = rng.standard_normal(L + 2000)
    if kind == 'fir':
        w = scipy.signal.lfilter([1.0, 0.9], [1.0], w)
    elif kind == 'butter4':
        w = scipy.signal.sosfilt(scipy.signal.butter(4, 0.5, output='sos'), w)
    elif kind == 'butter8' or kind.startswith('floor'):
        w = scipy.signal.sosfilt(scipy.signal.butter(8, 0.25, output='sos'), w)
    w = w[2000:]
    return w if kind.startswith('floor') else w / np.sqrt(np.mean(w * w))       # the floor is relative to unit-variance noise BEFORE the filter


def make_case(kind, L, nsrc=2, seed=0):
    """-> refs, ests (nsrc, L) float32.  kind in SPECTRA: references of that spectrum, each with L / 10 samples of exact silence (whose
    edges are broadband and keep cond(G) low); 'floor<amp>' (e.g. 'floor1e-5'): order-8 low-pass noise at 0.25 plus a white floor of that
    amplitude, no silence ('floor0': no floor at all, float32 rounding only).  Estimate j = a 200-tap filter of r_j + 300-tap filters of
    the other references + noise (floor cases: 40 / 48 taps and band-limited noise, see below)."""
    rng = np.random.default_rng([seed, SPECTRA.index(kind) if kind in SPECTRA else 7, L, nsrc])
    refs = np.stack([_shaped(rng, kind, L) for _ in range(nsrc)])
    if kind.startswith('floor'):
        # the Gram matrix is that of the FINITE signals: an abrupt first or last sample is a broadband event that alone holds cond(G)
        # near 1e6, so the low-pass part is faded in and out (Hann ramps) and only the floor is left to fill the stop band
        ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(500) / 500)
        refs[:, :500] *= ramp
        refs[:, -500:] *= ramp[::-1]
        refs = refs + float(kind[5:]) * rng.standard_normal(refs.shape)
    else:
        gap = L // 10
        for p in range(nsrc):
            at = (p + 1) * L // (nsrc + 2)
            refs[p, at:at + gap] = 0.0
    refs = refs.astype(np.float32)
    ests = np.zeros((nsrc, L))
    floor = kind.startswith('floor')
    for j in range(nsrc):
        for p in range(nsrc):
            n_tap = (40 if p == j else 48) if floor else (200 if p == j else 300)
            h = rng.standard_normal(n_tap) * np.exp(-np.arange(n_tap) / (10.0 if floor else 40.0)) * (0.3 if p == j else 0.08)
            h[0] += 1.0 if p == j else 0.25
            ests[j] += scipy.signal.lfilter(h, [1.0], refs[p].astype(np.float64))
        if floor:
            # what is left over shares the references' band and floor, as the output of an enhancer fed with the same recordings does
            # (SAR 29 to 37 dB).  White noise at -30 dB instead would sit 70 dB above the references' floor in their stop band; the weak
            # directions of G then carry it, and the two float64 ROUTES already differ by 2e-7 dB in SAR at flen 256 (measured; see
            # DESIGN 6d): the error of any Gram route grows as eps cond(G) N / L there, whatever computes it.
            ests[j] += 0.02 * _shaped(rng, kind, L) * np.concatenate([ramp, np.ones(L - 1000), ramp[::-1]]) + float(kind[5:]) * rng.standard_normal(L)
        else:
            ests[j] += 0.03 * rng.standard_normal(L)
    return refs, ests.astype(np.float32)


# ---- checks --------------------------------------------------------------------------------------------------------------------

def _bss(*a, **k):
    from disco_amd import metrics as dm
    return dm.bss_eval_sources(*a, **k)


def check_against_oracle(kinds, L, flen, nsrc=2, oracle='dense', cond_max=1e11):
    """Every case: cond(G) printed and asserted, every figure <= 40 dB, SDR / SIR / SAR of every source within TOL_DB of the oracle."""
    fn = dense_oracle if oracle == 'dense' else gram_oracle
    report = []
    for kind in kinds:
        refs, ests = make_case(kind, L, nsrc)
        cond = cond_gram(refs, flen)
        sdr, sir, sar, perm = _bss(refs, ests, compute_permutation=False, flen=flen)
        assert list(perm) == list(range(nsrc))
        worst = 0.0
        for j in range(nsrc):
            o = fn(refs, ests[j], j, flen)
            got = (sdr[j], sir[j], sar[j])
            for g, w in zip(got, o):
                if nsrc == 1 and not np.isfinite(w):
                    assert g == np.inf or g > 120, (kind, j, got, o)           # one source: nothing interferes
                    continue
                assert np.isfinite(g) and w <= 40.0, (kind, j, got, o)
                worst = max(worst, abs(g - w))
        print(f'bss {oracle} kind={kind} L={L} flen={flen} nsrc={nsrc} cond(G)={cond:.3g} sdr={sdr} sir={sir} sar={sar} worst |err|={worst:.3g} dB')
        assert cond <= cond_max, (kind, cond)
        assert worst < TOL_DB, (kind, flen, nsrc, worst)
        report.append((kind, cond, worst))
    return report


def check_closed_forms(L, flen):
    """White references (cond < 10)."""
    from disco_amd import metrics as dm
    rng = np.random.default_rng(11)
    refs = rng.standard_normal((2, L)).astype(np.float32)
    refs[0, -100:] = 0.0
    assert flen > 100 and cond_gram(refs, min(flen, 128)) < 10
    big = lambda v: v == np.inf or v > 120
    # estimate = r_0 exactly; a scaled, delayed copy of r_0 (nothing cut off: its last 100 samples are zero)
    delayed = np.zeros(L, np.float32)
    delayed[100:] = 3.0 * refs[0, :-100]
    for est0 in (refs[0], delayed):
        sdr, sir, sar, _ = _bss(refs, np.stack([est0, refs[1]]), compute_permutation=False, flen=flen)
        print('bss closed form: copy / delayed copy of r_0:', sdr[0], sir[0], sar[0])
        assert big(sdr[0]) and big(sir[0]) and big(sar[0]), (sdr, sir, sar)
    # estimate = r_0 + r_1: no artefacts, finite SDR and SIR
    mix = (refs[0].astype(np.float64) + refs[1]).astype(np.float32)
    sdr, sir, sar, _ = _bss(refs, np.stack([mix, mix]), compute_permutation=False, flen=flen)
    Ls = min(L, 4000)                                                    # the dense oracle on a span it can afford
    sdr_s, sir_s, sar_s, _ = _bss(refs, np.stack([mix, mix]), compute_permutation=False, flen=flen, stop=Ls)
    o = dense_oracle(refs[:, :Ls], mix[:Ls], 0, flen)
    print('bss closed form: r_0 + r_1:', sdr[0], sir[0], sar[0], 'on the first', Ls, 'samples', sdr_s[0], sir_s[0], sar_s[0], 'dense', o)
    assert big(sar[0]) and big(sar_s[0]) and np.isfinite(sdr[0]) and np.isfinite(sir[0])
    assert abs(sdr_s[0] - o[0]) < TOL_DB and abs(sir_s[0] - o[1]) < TOL_DB, (sdr_s, sir_s, o)
    # flen = 1, one source: the scale-invariant SDR of the existing module
    r1 = refs[:1]
    e1 = (r1.astype(np.float64) + 0.3 * rng.standard_normal((1, L))).astype(np.float32)
    sdr, sir, sar, _ = _bss(r1, e1, flen=1)
    ref = float(np.asarray(dm.si_sdr(r1[0], e1[0])))
    print('bss closed form: flen 1, one source:', sdr[0], 'si_sdr', ref)
    assert abs(sdr[0] - ref) < 1e-9 and abs(sar[0] - ref) < 1e-9 and sir[0] == np.inf


def check_permutation(L, flen):
    refs, ests = make_case('white', L, 3, seed=5)
    base = _bss(refs, ests, flen=flen)
    assert list(base[3]) == [0, 1, 2]
    plain = _bss(refs, ests, compute_permutation=False, flen=flen)
    for a, b in zip(base[:3], plain[:3]):
        assert np.array_equal(a, b)
    order = [2, 0, 1]                                                    # estimate slot i holds the estimate of source order[i]
    sw = _bss(refs, ests[order], flen=flen)
    assert list(sw[3]) == [order.index(j) for j in range(3)], sw[3]
    for a, b in zip(sw[:3], base[:3]):
        assert np.array_equal(a, b), (a, b)
    as_given = _bss(refs, ests[order], compute_permutation=False, flen=flen)
    assert list(as_given[3]) == [0, 1, 2] and np.all(as_given[1] < base[1] - 3), (as_given, base)     # wrong pairing: SIR collapses
    for j in range(3):
        o = dense_oracle(refs, ests[order][j], j, flen)
        assert abs(as_given[0][j] - o[0]) < TOL_DB and abs(as_given[1][j] - o[1]) < TOL_DB and abs(as_given[2][j] - o[2]) < TOL_DB
    print('bss permutation: perm', sw[3], 'sir', sw[1], 'as given', as_given[1])


def check_batching(L, flen, nsrc=2):
    from disco_amd import metrics as dm
    rng = np.random.default_rng(2)
    refs = rng.standard_normal((3, 5, nsrc, L)).astype(np.float32)
    ests = (refs + 0.2 * refs[..., ::-1, :] + 0.1 * rng.standard_normal(refs.shape)).astype(np.float32)
    for cp in (True, False):
        whole = _bss(refs, ests, compute_permutation=cp, flen=flen)
        assert all(v.shape == (3, 5, nsrc) for v in whole)
        again = _bss(refs, ests, compute_permutation=cp, flen=flen)
        for a, b in zip(whole, again):
            assert np.array_equal(a, b)                                  # run to run
        for i in range(3):
            for k in range(5):
                one = _bss(refs[i, k], ests[i, k], compute_permutation=cp, flen=flen)
                for a, b in zip(whole, one):
                    assert b.shape == (nsrc,) and np.array_equal(a[i, k], b), (i, k, a[i, k], b)
    eng = dm._engine()
    r3, e4 = refs.reshape(15, nsrc, L), ests.reshape(15, 1, nsrc, L)
    full, st_full = eng.bss_eval(r3, e4, flen=flen, all_pairs=True)
    per_set = eng.lib.disco_bss_workspace_bytes(eng.ctx, 1, nsrc, flen, L)
    for budget in (1, 4 * per_set + 1000):                               # one set per chunk; four per chunk with a ragged last chunk
        part, st_part = eng.bss_eval(r3, e4, flen=flen, all_pairs=True, budget_bytes=budget)
        assert np.array_equal(full, part) and np.array_equal(st_full, st_part) and not st_full.any()
    # several estimate sets against one factorisation = the same sets one by one
    e3 = np.ascontiguousarray(np.stack([e4[:, 0], e4[::-1, 0], r3], axis=1))
    many, _ = eng.bss_eval(r3, e3, flen=flen)
    for k in range(3):
        single, _ = eng.bss_eval(r3, np.ascontiguousarray(e3[:, k:k + 1]), flen=flen)
        assert np.array_equal(many[:, k], single[:, 0])
    print('bss batching: (3, 5) batch, chunked walks and 3 estimate sets bit-identical to the single calls')


def check_start_stop_and_lengths(L, flen):
    refs, ests = make_case('fir', L, 2, seed=3)
    a, b = L // 7, L - L // 5
    cut = _bss(np.ascontiguousarray(refs[:, a:b]), np.ascontiguousarray(ests[:, a:b]), flen=flen)
    span = _bss(refs, ests, flen=flen, start=a, stop=b)
    for x, y in zip(cut, span):
        assert np.array_equal(x, y), (x, y)
    # rooms of different clip lengths, zero-padded to a common length
    lens = [L, L - L // 3, L // 2]
    R = np.zeros((3, 2, L), np.float32)
    E = np.zeros((3, 2, L), np.float32)
    own = []
    for i, Li in enumerate(lens):
        r, e = make_case('white' if i else 'butter4', Li, 2, seed=20 + i)
        R[i, :, :Li], E[i, :, :Li] = r, e
        own.append(_bss(r, e, flen=flen))
    padded = _bss(R, E, flen=flen)
    worst = 0.0
    for i in range(3):
        assert np.array_equal(padded[3][i], own[i][3])
        worst = max(worst, max(float(np.max(np.abs(padded[q][i] - own[i][q]))) for q in range(3)))
    print('bss start / stop equal the sliced call; mixed lengths: worst |padded - own length| =', worst, 'dB')
    assert worst < 1e-9


def check_refusals(L, flens_lowpass=(64, 256)):
    import pytest
    from disco_amd import metrics as dm
    rng = np.random.default_rng(4)
    refs = rng.standard_normal((3, 2, L)).astype(np.float32)
    ests = (refs + 0.1 * rng.standard_normal(refs.shape)).astype(np.float32)
    good = _bss(refs, ests, flen=16)
    # an all-zero reference
    z = refs.copy()
    z[1, 1] = 0.0
    with pytest.raises(ValueError, match='reference source 1 of set .*1.* is all zero'):
        _bss(z, ests, flen=16)
    # a duplicated reference: NaN and status for that set alone, no exception
    d = refs.copy()
    d[1, 1] = d[1, 0]
    sdr, sir, sar, perm = _bss(d, ests, flen=16)
    assert np.all(np.isnan(sdr[1])) and np.all(np.isnan(sir[1])) and np.all(np.isnan(sar[1]))
    for i in (0, 2):
        for q, v in enumerate((sdr, sir, sar, perm)):
            assert np.array_equal(v[i], good[q][i])
    en, st = dm._engine().bss_eval(d, d[:, None], flen=16)
    assert list(st != 0) == [False, True, False] and np.all(np.isnan(en[1, ..., :3])) and np.all(en[1, ..., 3] == 1) and np.all(en[0, ..., 3] == 0)
    # references without a noise floor (cond(G) ~ 1e17): refused, or right -- never a wrong finite figure, never an exception
    for flen in flens_lowpass:
        r, e = make_case('floor0', 5000, 2, seed=9)
        en, st = dm._engine().bss_eval(r[None], e[None, None], flen=flen)
        sdr, sir, sar, _ = _bss(r, e, compute_permutation=False, flen=flen)
        if st[0]:
            print(f'bss floor-less low-pass references, flen {flen}: refused (status {st[0]})')
            assert np.all(np.isnan(sdr)) and np.all(np.isnan(sir)) and np.all(np.isnan(sar))
        else:
            worst = 0.0
            for j in range(2):
                o = dense_oracle(r, e[j], j, flen)
                worst = max(worst, abs(sdr[j] - o[0]), abs(sir[j] - o[1]), abs(sar[j] - o[2]))
            print(f'bss floor-less low-pass references, flen {flen}: status 0, worst |err| vs dense = {worst:.3g} dB')
            assert worst < 0.01, (flen, worst)
    # limits, named
    with pytest.raises(RuntimeError, match='nsrc <= 4'):
        _bss(rng.standard_normal((5, 400)).astype(np.float32), rng.standard_normal((5, 400)).astype(np.float32), flen=4)
    with pytest.raises(RuntimeError, match='flen <= 512'):
        _bss(refs[0], ests[0], flen=513)
    # shapes, before any launch
    with pytest.raises(ValueError):
        _bss(refs[0], ests[0][:, :-1])
    with pytest.raises(ValueError):
        _bss(refs[0], ests[:2])
    with pytest.raises(ValueError):
        dm._engine().bss_eval(refs, ests)
    with pytest.raises(RuntimeError):
        dm._engine().bss_eval(refs, ests[:, None], start=5, stop=L + 1, flen=4)
    with pytest.raises(RuntimeError):
        dm._engine().lag_corr(refs[0], refs[0], -512, 0)


def check_lag_corr(L):
    from disco_amd import metrics as dm
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((2, 3, L)).astype(np.float32)
    eng = dm._engine()
    for lo, hi, start, stop in ((-511, 511, 0, None), (0, 0, 0, None), (-3, 40, L // 9, L - 17), (5, 300, 1, L)):
        got = eng.lag_corr(a, b, lo, hi, start, stop).numpy()
        assert np.array_equal(got, eng.lag_corr(a, b, lo, hi, start, stop).numpy())
        sl = slice(start, stop)
        worst = 0.0
        for i in range(3):
            want = lag_corr_oracle(a[i, sl], b[i, sl], range(lo, hi + 1))
            worst = max(worst, float(np.max(np.abs(got[i] - want)) / np.sqrt((a[i, sl].astype(np.float64) ** 2).sum() * (b[i, sl].astype(np.float64) ** 2).sum())))
        print(f'lag_corr lags [{lo}, {hi}] span [{start}, {stop}): worst error / (|a| |b|) = {worst:.3g}')
        assert worst < 1e-14        # exact products, ~L additions in float64 in another order: sqrt(L) 1.1e-16 |a| |b| would be the random walk


def room_signals(K=2, L=16000 + 6000, seed=3):
    """A synthetic room shaped like the one of test_reference_surface_emulated.py::test_result_pickles, plus the mixture and the two
    enhanced mixtures."""
    rng = np.random.default_rng(seed)
    s_in, n_in = 0.1 * rng.standard_normal((K, L)), 0.05 * rng.standard_normal((K, L))
    sf_t, nf_t = 0.9 * s_in + 0.01 * rng.standard_normal((K, L)), 0.3 * n_in
    szf_t, nzf_t = 0.8 * s_in + 0.02 * rng.standard_normal((K, L)), 0.5 * n_in
    s_dry, n_dry = 0.2 * rng.standard_normal(L), 0.1 * rng.standard_normal(L)
    s_dry[200:] += 0.5 * s_in[0, :-200]                                   # the dry sources are not unrelated to what the nodes hear
    n_dry[150:] += 0.5 * n_in[0, :-150]
    f32 = lambda a: np.asarray(a, np.float32)
    d = dict(s_in=s_in, n_in=n_in, sf_t=sf_t, nf_t=nf_t, szf_t=szf_t, nzf_t=nzf_t, s_dry=s_dry, n_dry=n_dry, y_in=s_in + n_in,
             sh_t=sf_t + nf_t, szh_t=szf_t + nzf_t)
    return {k: f32(v) for k, v in d.items()}


def check_room_results(bss_flen, tmp_path, fs=16000, oracle='dense'):
    """Each of the eleven BSS keys, in both dictionaries, against the oracle applied as tango.py:541-567 reads."""
    import pickle
    from disco_amd.speech_enhancement import results_io as rio
    fn = dense_oracle if oracle == 'dense' else gram_oracle
    g = room_signals()
    K = g['s_in'].shape[0]
    kw = dict(rnd_snrs=[3.0], fs=fs)
    pos = [g[k] for k in ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')]
    res, resz = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], y_in=g['y_in'], sh_t=g['sh_t'], szh_t=g['szh_t'],
                                 bss_flen=bss_flen, **kw)
    assert tuple(res) == rio.RESULT_KEYS_TANGO and tuple(resz) == rio.RESULT_KEYS_MWF and len(rio.BSS_KEYS) == 11
    c64 = lambda a: a[..., fs:].astype(np.float64)
    y, sh, szh = c64(g['y_in']), c64(g['sh_t']), c64(g['szh_t'])
    f32 = lambda a: a.astype(np.float32)
    worst = 0.0
    for k in range(K):
        refs = np.stack([g['s_in'][k, fs:], g['n_in'][k, fs:]])
        refs_dry = np.stack([g['s_dry'][fs:], g['n_dry'][fs:]])
        est, est_z, est_i = f32(sh[k]), f32(szh[k]), f32(y[k])           # source 0's estimate of ests / ests_z / ests_i (tango.py:547-549)
        want = {}
        want['res', 'cnv'] = fn(refs, est, 0, bss_flen)
        want['resz', 'cnv'] = fn(refs, est_z, 0, bss_flen)
        want['both', 'in_cnv'] = fn(refs, est_i, 0, bss_flen)
        want['res', 'dry'] = fn(refs_dry, est, 0, bss_flen)
        want['resz', 'dry'] = fn(refs_dry, est_z, 0, bss_flen)
        want['both', 'in_dry'] = fn(refs_dry, est_i, 0, bss_flen)
        for (who, tag), o in want.items():
            for r in ((res, resz) if who == 'both' else (res,) if who == 'res' else (resz,)):
                for name, w in zip(('sdr', 'sir', 'sar'), o):
                    key = f'{name}_{tag}'
                    if key == 'sar_in_cnv':                              # not kept by the reference (tango.py:567)
                        assert key not in r
                        continue
                    assert w <= 40.0, (key, w)
                    worst = max(worst, abs(r[key][k] - w))
                    assert abs(r[key][k] - w) < TOL_DB, (key, k, r[key][k], w)
    for key in ('sdr_in_cnv', 'sir_in_cnv', 'sdr_in_dry', 'sir_in_dry', 'sar_in_dry'):
        assert np.array_equal(res[key], resz[key])
    for r in (res, resz):
        for key in r:
            assert len(r[key]) == K or key == 'snr_in_raw'
            if 'stoi' in key:
                assert np.all(np.isnan(r[key]))
        for key in rio.BSS_KEYS:
            assert np.all(np.isfinite(r[key])), key
    print(f'room_results BSS keys (flen {bss_flen}): worst |err| vs {oracle} = {worst:.3g} dB; sdr_cnv', res['sdr_cnv'], 'sdr_in_cnv', res['sdr_in_cnv'],
          'sdr_dry', res['sdr_dry'])
    # without the dry sources the _dry keys stay NaN; without the new arguments every BSS key is NaN, as before
    r2, rz2 = rio.room_results(*pos, y_in=g['y_in'], sh_t=g['sh_t'], szh_t=g['szh_t'], bss_flen=bss_flen, **kw)
    for key in rio.BSS_KEYS:
        assert np.all(np.isnan(r2[key])) == key.endswith('_dry'), key
        if not key.endswith('_dry'):
            assert np.array_equal(r2[key], res[key]) and np.array_equal(rz2[key], resz[key])
    r3, rz3 = rio.room_results(*pos, s_dry=g['s_dry'], n_dry=g['n_dry'], **kw)
    for key in rio.BSS_KEYS:
        assert np.all(np.isnan(r3[key])) and np.all(np.isnan(rz3[key]))
    files = rio.write_result_pickles(str(tmp_path), 11001, 'ssn', res, resz)
    for f, r in zip(files, (res, resz)):
        back = pickle.load(open(f, 'rb'))
        assert set(back) == set(r)
        for key in rio.BSS_KEYS:
            assert np.array_equal(back[key], r[key])


def make_c3_room(seed=0, K=4, M=4, L=160000):
    """One C3-shaped room with its dry sources (disco_amd.synth builds the same room but does not return them): white dry sources,
    synthetic RIRs (direct path + decaying tail), noise scaled to 0 ... 6 dB at node 0 -> y, s, n (K, M, L), s_dry, n_dry (L,) float32."""
    from disco_amd import synth
    rng = np.random.default_rng(4321 + seed)
    beta, dist, delay = synth._rir_params(rng, K, M)
    t = np.arange(synth.RIR_TAPS)
    rir = np.zeros((2, K, M, synth.RIR_TAPS))
    for src in range(2):
        for k in range(K):
            for m in range(M):
                d = int(delay[src, k, m])
                h = synth.TAIL_GAIN * rng.standard_normal(synth.RIR_TAPS) * np.exp(-6.9 * np.maximum(t - d, 0) / (beta * synth.FS))
                h[:d + 1] = 0.0
                if d < synth.RIR_TAPS:
                    h[d] = 1.0 / dist[src, k, m]
                rir[src, k, m] = h
    dry_s = (np.sqrt(synth.TARGET_VAR) * rng.standard_normal(L)).astype(np.float32)
    dry_n = rng.standard_normal(L).astype(np.float32)
    nfft = 1 << int(np.ceil(np.log2(L + synth.RIR_TAPS)))
    Hf = np.fft.rfft(rir, nfft, axis=-1)
    s_img = np.fft.irfft(np.fft.rfft(dry_s, nfft) * Hf[0], nfft, axis=-1)[..., :L]
    n_img = np.fft.irfft(np.fft.rfft(dry_n, nfft) * Hf[1], nfft, axis=-1)[..., :L]
    gain = np.sqrt(np.var(s_img[0, 0]) / (np.var(n_img[0, 0]) * 10 ** (rng.uniform(0, 6) / 10)))
    s32, n32 = s_img.astype(np.float32), (gain * n_img).astype(np.float32)
    return s32 + n32, s32, n32, dry_s, (gain * dry_n).astype(np.float32)


def check_c3_room_through_the_path(fs=16000, bss_flen=512, **room):
    """offline_tango -> iSTFT -> room_results with the BSS arguments, on one C3-shaped room (4 nodes x 4 microphones, 10 s, oracle masks)."""
    from disco_amd.math_utils import my_istft
    from disco_amd.speech_enhancement import results_io as rio
    from disco_amd.speech_enhancement.tango import offline_tango
    y, s, n, s_dry, n_dry = make_c3_room(**room)
    K, M, L = y.shape
    yf, sf, nf, z_y, z_s, z_n = offline_tango(list(y), list(s), list(n), vads=['irm1', 'irm1'])[:6]
    t = lambda spec: np.stack([my_istft(spec[k], L) for k in range(K)])
    sh_t, sf_t, nf_t, szh_t, szf_t, nzf_t = t(yf), t(sf), t(nf), t(z_y), t(z_s), t(z_n)
    res, resz = rio.room_results(s[:, 0], n[:, 0], sf_t, nf_t, szf_t, nzf_t, rnd_snrs=[0.0], s_dry=s_dry, n_dry=n_dry, fs=fs,
                                 y_in=y[:, 0], sh_t=sh_t, szh_t=szh_t, bss_flen=bss_flen)
    for r in (res, resz):
        for key in rio.BSS_KEYS:
            assert r[key].shape == (K,) and np.all(np.isfinite(r[key])), (key, r[key])
    f32 = lambda a: np.asarray(a, np.float32)
    for k in range(K):
        refs = np.stack([s[k, 0, fs:], n[k, 0, fs:]])
        est = np.stack([sh_t[k, fs:], f32(y[k, 0, fs:].astype(np.float64) - sh_t[k, fs:])])
        sdr, sir, sar, _ = _bss(refs, f32(est), compute_permutation=False, flen=bss_flen)
        assert sdr[0] == res['sdr_cnv'][k] and sir[0] == res['sir_cnv'][k] and sar[0] == res['sar_cnv'][k], (k, sdr, res['sdr_cnv'])
    print('C3-shaped room through the path: sdr_in_cnv', res['sdr_in_cnv'], '-> sdr_cnv step 1', resz['sdr_cnv'], 'step 2', res['sdr_cnv'],
          '; change in SDR (step 2 - input)', res['sdr_cnv'] - res['sdr_in_cnv'], '; sir_cnv', res['sir_cnv'], 'sar_cnv', res['sar_cnv'],
          '; sdr_in_dry', res['sdr_in_dry'], 'sdr_dry', res['sdr_dry'])
