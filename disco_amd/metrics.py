"""Evaluation metrics with the reference's names (disco_theque/metrics.py), batched and computed on the GPU.

Every function takes arrays whose LAST axis is time and whose leading axes are a batch (rooms, nodes, ...): NumPy arrays
(copied to the device) or device-resident torch tensors / DevBufs of shape (n_sig, L) (zero-copy).  The time signals never
come back to the host: the HIP kernels (csrc/k_metrics.h) reduce them to a few float64 moments per signal and the dB /
clipping / importance-weight arithmetic of the reference is applied to those.

    snr, delta_snr, sd        metrics.py:9-61       variance of the NON-ZERO samples, as the reference
    fw_snr, fw_sd             metrics.py:63-128, 211-279   (third-octave Butterworth bank, clip, band-importance weights)
    seg_snr                   metrics.py:131-173      (clipped level ratio of every whole window, VAD-weighted; csrc/k_segsnr.h)
    reverb_ratios             metrics.py:176-208      (DRR and SRR of dry signals through RIRs; csrc/k_reverb.h: the two convolutions
                              are reduced to their energies without being written)
    ci_wp                     metrics.py:283-288      (host NumPy on a handful of numbers; misc_utils.bar_data is its caller)
    si_sdr                    metrics.py:342-391
    si_bss                    metrics.py:282-340      (SI-SDR / SI-SIR / SI-SAR against n_src references)
    bss_eval_sources          mir_eval.separation.bss_eval_sources as tango.py:541-567 calls it (SDR / SIR / SAR through a 512-tap
                              filtered projection; third-party and absent here: restated from its definition, csrc/k_bss.h)
    stoi                      pystoi.stoi as tango.py:569-578 calls it (third-party and absent here: restated from its definition with
                              pystoi's constants, csrc/k_stoi.h; pinned by the float64 yardstick of tests/stoi_checks.py, unpinned
                              against the package)
    estoi                     the extended STOI of Jensen & Taal 2016, pystoi.stoi(..., extended=True) without its random jitter
                              (csrc/k_estoi.h; pinned by the float64 yardstick of tests/estoi_checks.py)
    third_octave_filterbank   sigproc_utils.py:90-116

`start` / `stop` select the scored span; the reference scores [fs : min_len] (tango.py:541-593), i.e. start = 16000.
Batches with per-room lengths (Engine.set_lengths): every metric takes a stop per signal.  `stop` is None (the whole last axis), a
scalar, or an array shaped like (or broadcastable to) the leading axes -- for bss_eval_sources the leading axes before `nsrc`.  Signal
i is then scored over [start, stop[i]) exactly as if it had been sliced and scored alone: its band filters stop at its own end, so
the ringing past a clip is never scored, and nothing at or beyond stop[i] is read -- the padding may hold anything, NaN included.
speech_enhancement.results_io.batch_results scores a whole batch of rooms this way in one call.
Band edges: the reference takes them from python-acoustics' OctaveBand (third-party, absent); they are restated from
IEC 61260-1 (base-10 octave ratio, exact mid-band frequencies) -- the one unpinned piece, see oracle/metrics_oracle.py.
"""
import itertools

import numpy as np
import scipy.signal

from ._engines import get_engine

_G = 10.0 ** 0.3
_F_WB = np.array([160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000])
_I_WB = np.array([83, 95, 150, 289, 440, 578, 653, 711, 818, 844, 882, 898, 868, 844, 771, 527, 364, 185]) * 1e-4
_F_NB = np.array([200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000])
_I_NB = np.array([128, 320, 320, 447, 447, 639, 639, 767, 959, 1182, 1214, 1086, 1086, 757]) * 1e-4


def lin2db(x):
    return 10 * np.log10(x)


def _engine():
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)      # metrics kernels do not depend on the batch geometry


def _flat(x):
    """-> (2-D view (n_sig, L), leading shape)."""
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float32)
        return x.reshape(-1, x.shape[-1]), x.shape[:-1]
    shape = tuple(x.shape)
    return x.reshape(-1, shape[-1]) if hasattr(x, 'reshape') else x, shape[:-1]


def _var_nz(cnt, s1, s2):
    mean = s1 / cnt
    return s2 / cnt - mean * mean                                # np.var (ddof 0) of the non-zero samples


def _span_stops(stop, lead):
    """`stop` of a metric -> None / a scalar unchanged, or one stop per flattened signal: an array broadcast over the leading axes."""
    if stop is None or not np.ndim(stop):
        return stop
    try:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(stop), tuple(lead))).reshape(-1)
    except ValueError:
        raise ValueError(f'stop of shape {np.shape(stop)} does not broadcast to the leading axes {tuple(lead)}') from None


def _levels(x, start, stop):
    x2, lead = _flat(x)
    st = _engine().pair_stats(x2, x2, start, _span_stops(stop, lead)).numpy()
    return _var_nz(st[:, 0], st[:, 1], st[:, 2]).reshape(lead)


def snr(s, n, db=True, start=0, stop=None):
    """metrics.py:9-24"""
    v = _levels(s, start, stop) / _levels(n, start, stop)
    return lin2db(v) if db else v


def delta_snr(s_out, n_out, s_in, n_in, db=True, start=0, stop=None):
    """metrics.py:27-45"""
    d = snr(s_out, n_out, True, start, stop) - snr(s_in, n_in, True, start, stop)
    return d if db else 10 ** (d / 10)


def sd(s_out, s_in, db=True, start=0, stop=None):
    """metrics.py:48-61"""
    v = _levels(s_in, start, stop) / _levels(s_out, start, stop)
    return lin2db(v) if db else v


def _as_signals(x):
    """A NumPy array (or anything np.asarray takes) -> contiguous float32; a device tensor / DevBuf as it is."""
    if isinstance(x, np.ndarray) or not (hasattr(x, 'data_ptr') or hasattr(x, 'ptr')):
        return np.ascontiguousarray(x, dtype=np.float32)
    return x


def seg_snr(s, n, win_len, win_hop, vad=None, start=0, stop=None):
    """metrics.py:131-173, batched over the leading axes: -> one value per signal pair in dB (a float for 1-D inputs).
    Over the span [start, stop[i]) of L_i samples, windows m = 0 .. N_w - 1 cover [start + m win_hop, start + m win_hop + win_len) with
    N_w = (L_i - win_len) // win_hop + 1 (whole windows only; none when L_i < win_len).  Per window and signal the variance is np.var in
    float64 on the float32 samples, floored at sys.float_info.epsilon; v_m = clip(10 log10(var_s / var_n), -15, 25); the result is
    sum g_m v_m / sum g_m with g_m = 1, or, with a VAD, g_m = vad[i][start + m win_hop] (the value itself, not a non-zero test).
    vad is per SAMPLE and shaped like s: what sigproc_utils.vad_oracle_batch returns.  The reference takes one value per window from a
    `db_utils.frame_vad` it does not ship; the decimation used here is the one the reference itself applies to a per-sample VAD for its
    'ivad' masks (tango.py:219-220, vad[::N_HOP]).  The log, the clip and the sums happen in the kernel (Engine.seg_snr,
    csrc/k_segsnr.h); two numbers per signal are divided here.
    NaN where N_w = 0 or sum g_m = 0 (the reference divides by zero there).  s and n must have equal shapes: unequal shapes raise
    ValueError -- the reference's reflect-padding of the shorter signal is not offered.  win_len <= 2048."""
    s, n = _as_signals(s), _as_signals(n)
    shape = tuple(int(v) for v in s.shape)
    if len(shape) < 1 or tuple(int(v) for v in n.shape) != shape:
        raise ValueError(f's and n must have the same shape, found {shape} and {tuple(n.shape)} (no reflect-padding of the shorter one here)')
    if vad is not None:
        vad = _as_signals(vad)
        if tuple(int(v) for v in vad.shape) != shape:
            raise ValueError(f'vad must be per sample and shaped like s, {shape}: found {tuple(vad.shape)}')
    lead, L = shape[:-1], shape[-1]
    n_sig = int(np.prod(lead, dtype=np.int64))
    if L == 0 or n_sig == 0:                                     # nothing to read: no window anywhere
        return np.full(lead, np.nan) if lead else float('nan')
    flat = lambda a: a.reshape(n_sig, L)
    st = _engine().seg_snr(flat(s), flat(n), int(win_len), int(win_hop), None if vad is None else flat(vad), int(start),
                           _span_stops(stop, lead)).numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        v = np.where(st[:, 2] > 0, st[:, 0] / st[:, 1], np.nan)
    return v.reshape(lead) if lead else float(v[0])


def reverb_ratios(x, rir, reverb_start=20, fs=16000):
    """metrics.py:176-208, batched: x (n_sig, Ld) dry signals, rir (n_sig, n_ch, rir_len), rir_len <= 8192 -> (drr, srr) in dB, each
    (n_sig, n_ch); a 1-D x with a 1-D rir (the reference's own call) -> two floats.
        split = min(argmax(rir) + n_d, rir_len), n_d = int(1e-3 reverb_start fs)     (argmax of the signed response, first maximum)
        h_d = rir[:split], h_r = rir[split:];  drr = 10 log10(sum h_d^2 / sum h_r^2);  srr = 10 log10(sum (x * h_d)^2 / sum (x * h_r)^2)
    over the full convolutions, energies in float64 (Engine.rir_split, Engine.reverb_energies: csrc/k_reverb.h; neither convolution is
    written to memory).  An empty tail (split == rir_len) gives +inf for both; the reference raises ValueError from np.convolve there,
    which a batch cannot do for one of its rows."""
    x, rir = _as_signals(x), _as_signals(rir)
    one = len(x.shape) == 1 and len(rir.shape) == 1
    if one:
        x, rir = x.reshape(1, -1), rir.reshape(1, 1, -1)
    if len(x.shape) != 2 or len(rir.shape) != 3 or int(rir.shape[0]) != int(x.shape[0]):
        raise ValueError(f'x must be (n_sig, Ld) and rir (n_sig, n_ch, rir_len), or both 1-D: {tuple(x.shape)} and {tuple(rir.shape)}')
    eng = _engine()
    split, e_h = eng.rir_split(rir, int(1e-3 * reverb_start * fs))
    e_x = eng.reverb_energies(x, rir, split).numpy()
    drr, srr = _ratio_db(e_h.numpy()), _ratio_db(e_x)
    return (float(drr[0, 0]), float(srr[0, 0])) if one else (drr, srr)


def _ratio_db(e):
    """(..., 2) energies -> 10 log10(e[..., 0] / e[..., 1]): +inf for an empty tail, -inf for an empty direct part, NaN for 0 / 0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10 * np.log10(e[..., 0] / e[..., 1])


def ci_wp(x, axis=0):
    """metrics.py:283-288: the 95 % confidence half-width 1.96 nanstd(x) / sqrt(n) along `axis` (host NumPy, as the reference)."""
    return 1.96 * np.nanstd(x, axis=axis) / np.sqrt(np.shape(x)[axis])


def si_sdr(reference, estimation, start=0, stop=None):
    """metrics.py:342-391 (batched over the leading axes)."""
    r2, lead = _flat(reference)
    e2, _ = _flat(estimation)
    st = _engine().pair_stats(r2, e2, start, _span_stops(stop, lead)).numpy()
    e_ref, e_est, dot = st[:, 2], st[:, 5], st[:, 6]
    proj = dot * dot / e_ref                                       # |alpha ref|^2
    return (10 * np.log10(proj / (e_est - proj))).reshape(lead)


def si_bss(estimated_signal, targets, j, scaling=True, start=0, stop=None):
    """metrics.py:282-340, batched: estimated_signal (..., L), targets (n_src, ..., L) -> (sisdr, sisir, sisar), each (...).
    Everything the reference computes is a function of the Gram matrix of (estimate, targets); its entries are the cross
    moments `disco_pair_stats` returns, so no residual signal is ever formed."""
    e2, lead = _flat(estimated_signal)
    tg = [_flat(t)[0] for t in targets]
    n_src = len(tg)
    eng = _engine()
    stop = _span_stops(stop, lead)
    dot = lambda a, b: eng.pair_stats(a, b, start, stop).numpy()[:, 6]
    Rss = np.empty((e2.shape[0], n_src, n_src))
    for p in range(n_src):
        for q in range(p, n_src):
            Rss[:, p, q] = Rss[:, q, p] = dot(tg[p], tg[q])
    r_e = np.stack([dot(tg[p], e2) for p in range(n_src)], axis=1)            # targets^T estimate
    ee = eng.pair_stats(e2, e2, start, stop).numpy()[:, 2]
    a = r_e[:, j] / Rss[:, j, j] if scaling else np.ones(e2.shape[0])
    Sss = a * a * Rss[:, j, j]
    Snn = ee - 2 * a * r_e[:, j] + Sss                                        # |est - a s_j|^2
    Rsr = r_e - a[:, None] * Rss[:, :, j]                                     # targets^T e_res
    b = np.linalg.solve(Rss, Rsr[..., None])[..., 0]
    interf = np.einsum('np,np->n', b, Rsr)                                    # |targets b|^2 = b^T Rss b = b^T Rsr
    artif = Snn - interf                                                      # |e_res - e_interf|^2
    f = lambda x: (10 * np.log10(x)).reshape(lead)
    return f(Sss / Snn), f(Sss / interf), f(Sss / artif)


def _safe_db(num, den):
    """10 log10(num / den), +inf where den == 0 (mir_eval's _safe_db)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den == 0, np.inf, 10 * np.log10(num / np.where(den == 0, 1.0, den)))


def _figures(en):
    """Engine.bss_eval energies (..., 4) = {p_j, p_all, ee, status} -> (sdr, sir, sar), each (...): mir_eval's arithmetic; NaN energies
    (a refused set) give NaN."""
    pj, pall, ee = en[..., 0], en[..., 1], en[..., 2]
    nan = np.isnan(pj) | np.isnan(pall) | np.isnan(ee)
    pj, pall, ee = (np.where(nan, 1.0, v) for v in (pj, pall, ee))
    with np.errstate(divide='ignore'):
        sdr = _safe_db(pj, np.maximum(ee - pj, 0.0))
        sir = _safe_db(pj, np.maximum(pall - pj, 0.0))
        sar = _safe_db(pall, np.maximum(ee - pall, 0.0))
    return tuple(np.where(nan, np.nan, v) for v in (sdr, sir, sar))


def _raise_on_zero_reference(refs, status, start=0, stop=None, lead=None):
    """refs (n_set, nsrc, L), status of Engine.bss_eval: ValueError naming the first all-zero reference of a refused set, if there is one."""
    if not np.any(status != 0):
        return
    n_set, nsrc, L = (int(v) for v in refs.shape)
    r2 = refs.reshape(n_set * nsrc, L)
    if stop is not None and np.ndim(stop):                                    # one stop per set: every source of the set shares it
        stop = np.repeat(np.asarray(stop).reshape(n_set), nsrc)
    e_ref = _engine().pair_stats(r2, r2, start, stop).numpy()[:, 2]
    zero = np.flatnonzero(e_ref == 0)
    if zero.size:
        i = int(zero[0])
        where = tuple(int(v) for v in np.unravel_index(i // nsrc, lead)) if lead else (i // nsrc,)
        raise ValueError(f'reference source {i % nsrc} of set {where} is all zero over the scored span')


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True, start=0, stop=None, flen=512):
    """mir_eval.separation.bss_eval_sources (name, argument order, default): -> (sdr, sir, sar, perm).
    reference_sources, estimated_sources: (nsrc, L) as in mir_eval -> four (nsrc,) arrays, or (..., nsrc, L) batched over the leading
    axes -> (..., nsrc); NumPy arrays (copied) or device-resident (n_set, nsrc, L) tensors (read in place).  nsrc <= 4, flen <= 512.
    The estimate is projected on the `flen` delayed copies of its target reference (energy p_j) and on those of all references (p_all),
    through the lag correlations, one Cholesky factorisation per reference set and a forward substitution per estimate on the GPU
    (Engine.bss_eval); the arithmetic below on three float64 energies per figure is mir_eval's:
        SDR = 10 log10(p_j / (ee - p_j))   SIR = 10 log10(p_j / (p_all - p_j))   SAR = 10 log10(p_all / (ee - p_all))
    with the differences clamped at 0 from below and +inf for a zero denominator.  compute_permutation=True scores every (estimate,
    source) pair and returns, per source j, the figures of estimate perm[j] for the permutation with the best mean SIR; False (what
    tango.py passes) scores estimate j against source j and returns perm = arange(nsrc).
    `start` / `stop` select the scored span; `stop` may be an array shaped like the leading axes (one stop per reference set), so that a
    batch of different clip lengths scores every set as if it ran alone, whatever the samples past its clip hold.
    An all-zero reference raises ValueError naming the signal.  Where the references of a set are linearly dependent, or their Gram
    matrix is singular to working precision, that set's figures are NaN (mir_eval falls back to a least-squares solve there)."""
    refs, ests = reference_sources, estimated_sources
    if isinstance(refs, np.ndarray) or not hasattr(refs, 'data_ptr'):
        refs = np.ascontiguousarray(refs, dtype=np.float32)
    if isinstance(ests, np.ndarray) or not hasattr(ests, 'data_ptr'):
        ests = np.ascontiguousarray(ests, dtype=np.float32)
    shape = tuple(int(v) for v in refs.shape)
    if len(shape) < 2 or tuple(int(v) for v in ests.shape) != shape:
        raise ValueError(f'reference_sources and estimated_sources must have one shape (..., nsrc, L): {shape} and {tuple(ests.shape)}')
    lead, nsrc, L = shape[:-2], shape[-2], shape[-1]
    n_set = int(np.prod(lead, dtype=np.int64))
    eng = _engine()
    r3 = refs.reshape(n_set, nsrc, L)
    stop = _span_stops(stop, lead)
    en, status = eng.bss_eval(r3, ests.reshape(n_set, 1, nsrc, L), start, stop, flen, all_pairs=bool(compute_permutation))
    _raise_on_zero_reference(r3, status, start, stop, lead)
    sdr, sir, sar = _figures(en[:, 0])                                    # (n_set, nsrc[, nsrc])
    idx = np.arange(nsrc)
    if compute_permutation:                                               # [estimate][source], as mir_eval's sdr[jest, jtrue]
        perms = np.array(list(itertools.permutations(range(nsrc))))
        mean_sir = np.stack([sir[:, p, idx].mean(axis=1) for p in perms], axis=1)          # (n_set, n_perm)
        best = np.argmax(np.where(np.isnan(mean_sir), -np.inf, mean_sir), axis=1)
        perm = perms[best]                                                # (n_set, nsrc)
        rows = np.arange(n_set)[:, None]
        sdr, sir, sar = sdr[rows, perm, idx], sir[rows, perm, idx], sar[rows, perm, idx]
    else:
        perm = np.broadcast_to(idx, (n_set, nsrc)).copy()
    return tuple(v.reshape(lead + (nsrc,)) for v in (sdr, sir, sar, perm))


def stoi(x, y, fs_sig, extended=False, start=0, stop=None):
    """pystoi.stoi (name, argument order): x clean, y processed, (L,) -> float, or (..., L) batched over the leading axes -> (...);
    NumPy arrays (copied) or device-resident (n_pair, L) tensors (read in place).  Both are resampled to 10 kHz, the frames of x more
    than 40 dB below its loudest are removed from both, and the third-octave envelopes of every 30-frame segment are normalised,
    clipped and correlated, all on the GPU (Engine.stoi, csrc/k_stoi.h).  `start` / `stop` select the scored span; `stop` may be an
    array shaped like the leading axes, so that a batch of different clip lengths scores every pair as if it ran alone.
    Fewer than 30 frames after the removal: 1e-5 and a RuntimeWarning, as pystoi.  A span too short for a single frame (fewer than 257
    samples at 10 kHz) raises ValueError naming the pair.  extended=True raises NotImplementedError: the extended measure is `estoi`,
    a function of its own because it leaves out the random jitter of pystoi's variant."""
    if extended:
        raise NotImplementedError('extended=True is not offered here: call disco_amd.metrics.estoi (ESTOI without the random jitter of pystoi)')
    return _stoi_family('stoi', x, y, fs_sig, start, stop)


def estoi(x, y, fs_sig, start=0, stop=None):
    """ESTOI, the extended STOI of Jensen & Taal 2016 (what pystoi.stoi computes with extended=True): the arguments, shapes, warning and
    errors of `stoi`.  Resampling, silent-frame removal and the third-octave envelopes are STOI's; every 15 x 30 segment is normalised by
    rows and then by columns, without clipping, and the column correlations are averaged, all on the GPU (Engine.estoi, csrc/k_estoi.h).
    Restated from the definition and pinned by the float64 yardstick of tests/estoi_checks.py, unpinned against the package.  pystoi adds
    EPS randn before each normalisation so that it never divides by zero; that jitter is not reproduced (it moves d by some 1e-15 on
    the cases of tests/estoi_checks.py): the result is deterministic, and a row or column whose centred norm is exactly 0 contributes 0."""
    return _stoi_family('estoi', x, y, fs_sig, start, stop)


def _stoi_family(which, x, y, fs_sig, start, stop):
    """`stoi` and `estoi`: Engine.<which> over the flattened leading axes, the warning and the error."""
    if isinstance(x, np.ndarray) or not hasattr(x, 'data_ptr'):
        x = np.ascontiguousarray(x, dtype=np.float32)
    if isinstance(y, np.ndarray) or not hasattr(y, 'data_ptr'):
        y = np.ascontiguousarray(y, dtype=np.float32)
    shape = tuple(int(v) for v in x.shape)
    if len(shape) < 1 or tuple(int(v) for v in y.shape) != shape:
        raise ValueError(f'x and y should have the same length, found {shape} and {tuple(y.shape)}')
    lead, L = shape[:-1], shape[-1]
    n_pair = int(np.prod(lead, dtype=np.int64))
    if stop is not None and np.ndim(stop):
        stop = np.broadcast_to(np.asarray(stop), lead).reshape(n_pair)
    d, status = getattr(_engine(), which)(x.reshape(n_pair, L), y.reshape(n_pair, L), fs_sig, start, stop)
    if np.any(status == 2):
        i = int(np.flatnonzero(status == 2)[0])
        where = tuple(int(v) for v in np.unravel_index(i, lead)) if lead else ()
        raise ValueError(f'pair {where}: the scored span is too short for one frame (fewer than 257 samples at 10 kHz)')
    if np.any(status == 1):
        import warnings
        warnings.warn('Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. '
                      'Returning 1e-5. Please check you wav files', RuntimeWarning)
    return d.reshape(lead) if lead else float(d[0])


def band_importance(fs):
    """metrics.py:80-97: centre frequencies whose upper edge lies below fs/2, and their importance weights."""
    F, I = (_F_WB, _I_WB) if fs / 2 > 4500 else (_F_NB, _I_NB)
    N = int(np.sum(F * 2 ** (1 / 6) < fs / 2))
    return F[:N], I[:N]


def third_octave_filterbank(F, fs, order=8):
    """sigproc_utils.py:90-116: Butterworth band-pass per third-octave band, 'ba' form."""
    n = np.round(3 * np.log(np.asarray(F, float) / 1000.0) / np.log(_G))
    fc = 1000.0 * _G ** (n / 3)
    lo, hi = fc * _G ** (-1 / 6), fc * _G ** (1 / 6)
    b = np.zeros((len(F), 2 * order + 1))
    a = np.zeros((len(F), 2 * order + 1))
    for i in range(len(F)):
        b[i], a[i] = scipy.signal.butter(order, np.array([lo[i], hi[i]]) * 2 / fs, btype='bandpass', output='ba')
    return b, a


def _band_levels(x, b, a, start, stop, gate=None):
    x2, lead = _flat(x)
    g2 = None
    if gate is not None:
        if isinstance(gate, np.ndarray) or not (hasattr(gate, 'data_ptr') or hasattr(gate, 'ptr')):       # a host array (not a tensor, not a DevBuf)
            gate = np.broadcast_to(np.asarray(gate, dtype=np.float32), lead + (x2.shape[-1],))       # one VAD for the whole batch is fine
        g2, _ = _flat(gate)
    st = _engine().band_stats(x2, b, a, start, _span_stops(stop, lead), gate=g2).numpy()
    return _var_nz(st[..., 0], st[..., 1], st[..., 2]).reshape(lead + (b.shape[0],))


def _band_levels2(x, y, b, a, start, stop):
    """Levels of two equally shaped batches in ONE launch: the recurrences are sequential in time, so the only parallelism
    is (signal, band) -- stacking both batches doubles the waves in flight."""
    x2, lead = _flat(x)
    y2, lead_y = _flat(y)
    if lead != lead_y or type(x2) is not type(y2) or hasattr(x2, 'ptr'):          # (two DevBufs cannot be stacked: one launch each)
        return _band_levels(x, b, a, start, stop), _band_levels(y, b, a, start, stop)
    if isinstance(x2, np.ndarray):
        both = np.concatenate([x2, y2], 0)
    else:
        import torch
        both = torch.cat([x2, y2], 0)
    stop = _span_stops(stop, lead)
    if stop is not None and np.ndim(stop):
        stop = np.concatenate([stop, stop])
    lv = _band_levels(both, b, a, start, stop)
    n = x2.shape[0]
    return lv[:n].reshape(lead + (b.shape[0],)), lv[n:].reshape(lead + (b.shape[0],))


def fw_snr(s, n, fs, vad_tar=None, vad_noi=None, clipping=1, db=True, start=0, stop=None):
    """metrics.py:63-128 -> (fw_snr per band, mean, centre frequencies); leading axes batched.  vad_tar / vad_noi (shaped like s / n, or
    (L,) for the whole batch): the band levels are the variances of the filtered samples where the VAD is non-zero (metrics.py:104-112)
    instead of where the filtered sample is non-zero; they are indexed like the signals (`start` / `stop` cut both)."""
    F, I = band_importance(fs)
    b, a = third_octave_filterbank(F, fs, order=4)
    if vad_tar is None and vad_noi is None:
        ls, ln = _band_levels2(s, n, b, a, start, stop)
    else:
        ls, ln = _band_levels(s, b, a, start, stop, gate=vad_tar), _band_levels(n, b, a, start, stop, gate=vad_noi)
    fq, mean = _weighted_band_db(ls, ln, I, -15 if clipping else None)
    return (fq, mean, F) if db else (10 ** (fq / 10), 10 ** (mean / 10), F)


def _weighted_band_db(num, den, I, floor):
    """Band levels (..., n_bands) -> (importance-weighted level ratio per band in dB, its sum over the bands): the arithmetic fw_snr
    (floor -15) and fw_sd (floor 0) share, metrics.py:113-127, 262-278; floor None: no clipping."""
    v = lin2db(num) - lin2db(den)
    if floor is not None:
        v = np.minimum(np.maximum(floor, v), 25)
    fq = I / np.sum(I) * v
    return fq, np.sum(fq, axis=-1)


def fw_sd(s_out, s_in, fs, clipping=1, db=True, start=0, stop=None):
    """metrics.py:211-279"""
    F, I = band_importance(fs)
    b, a = third_octave_filterbank(F, fs, order=4)
    li, lo = _band_levels2(s_in, s_out, b, a, start, stop)
    fq, mean = _weighted_band_db(li, lo, I, 0 if clipping else None)
    return (fq, mean, F) if db else (10 ** (fq / 10), 10 ** (mean / 10), F)
