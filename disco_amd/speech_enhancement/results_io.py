"""The audio / mask files the reference writes after the path (disco_theque/speech_enhancement/tango.py:595-613), for batches:

    <root>/WAV/<i_rir>/in_mix-<noise>_Node-<k>.wav      y[k][0]          mixture at the node's first microphone
    <root>/WAV/<i_rir>/out_mix-<noise>_Node-<k>.wav     iSTFT(yf)        step-2 output
    <root>/WAV/<i_rir>/mid_z-<noise>_Node-<k>.wav       iSTFT(z_y)       compressed signal after step 1
    <root>/WAV/<i_rir>/in_noi- / out_noi- / in_tar- / out_tar-<noise>_Node-<k>.wav     n[k][0], iSTFT(nf), s[k][0], iSTFT(sf)
    <root>/MASK/<i_rir>/step1_<noise>_Node-<k>.npy, step2_...npy                        masks_z, mask_w   (F, T)

The reference writes the audio with `soundfile.write(path, data, fs)` (third-party, absent): for a '.wav' path and float
input that is 16-bit PCM, full scale at +-1.0.  Here the standard library's `wave` module writes the same container
(samples = round(clip(x, -1, 1 - 2^-15) * 32768)); bit-level equality with libsndfile's rounding is not pinned.

And the two result pickles of tango.py:617-635 (`room_results`, `write_result_pickles`): the level metrics and, given the mixture and
the two enhanced mixtures in time, the eleven BSS-eval keys (SDR / SIR / SAR, what the reference takes from mir_eval) and, with `stoi=True`, the three
STOI keys (what it takes from pystoi), all scored on the GPU by disco_amd.metrics.
"""
import os
import wave

import numpy as np

FS = 16000
WAV_KINDS = ('in_mix', 'out_mix', 'mid_z', 'in_noi', 'out_noi', 'in_tar', 'out_tar')


def write_wav(path, x, fs=FS):
    """float signal in [-1, 1) -> 16-bit PCM mono WAV."""
    x = np.asarray(x, dtype=np.float64)
    pcm = np.round(np.clip(x, -1.0, 1.0 - 2.0 ** -15) * 32768.0).astype('<i2')
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(fs))
        f.writeframes(pcm.tobytes())


def read_wav(path):
    with wave.open(path, 'rb') as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        fs = f.getframerate()
        x = np.frombuffer(f.readframes(f.getnframes()), dtype='<i2').astype(np.float32) / 32768.0
    return x, fs


def write_room_results(root, i_rir, noise, signals, masks_z=None, mask_w=None, fs=FS):
    """signals: dict kind -> (K, L) array for kinds of WAV_KINDS (missing kinds are skipped); masks (K, T, F) engine layout
    (written transposed, (F, T), as the reference holds them).  Returns the list of files written."""
    wav_dir = os.path.join(root, 'WAV', str(i_rir))
    os.makedirs(wav_dir, exist_ok=True)
    written = []
    for kind in WAV_KINDS:
        if kind not in signals:
            continue
        arr = np.asarray(signals[kind])
        for k in range(arr.shape[0]):
            p = os.path.join(wav_dir, '{}-{}_Node-{}.wav'.format(kind, noise, k + 1))
            write_wav(p, arr[k], fs)
            written.append(p)
    if masks_z is not None or mask_w is not None:
        mdir = os.path.join(root, 'MASK', str(i_rir))
        os.makedirs(mdir, exist_ok=True)
        for name, m in (('step1', masks_z), ('step2', mask_w)):
            if m is None:
                continue
            m = np.asarray(m)
            for k in range(m.shape[0]):
                p = os.path.join(mdir, '{}_{}_Node-{}.npy'.format(name, noise, k + 1))
                np.save(p, np.ascontiguousarray(m[k].T))
                written.append(p)
    return written


# ---- the result pickles (tango.py:617-635) ------------------------------------------------------------------------------------
# Two dictionaries of per-node arrays per (room, noise): `results_tango_<rir>_<noise>.p` (step-2 output) and
# `results_mwf_<rir>_<noise>.p` (the compressed signal after step 1), same keys as the reference.  The level metrics (fw_snr,
# fw_sd: the reference's own disco_theque/metrics.py) are computed by disco_amd.metrics on the GPU.  The eleven keys the reference
# fills from mir_eval.separation.bss_eval_sources (BSS_KEYS) are computed on the GPU too, by disco_amd.metrics.bss_eval_sources
# (restated from the definition of BSS-eval; mir_eval itself is third-party and absent), when room_results is given the time
# signals they need (y_in, sh_t, szh_t); without them they hold NaN.  The keys the reference fills from pystoi.stoi (STOI_KEYS) are
# computed by disco_amd.metrics.stoi (restated from the definition of STOI with pystoi's constants; the package is third-party, absent
# and the restatement unpinned against it) when room_results is given the same signals and `stoi=True`; otherwise they are present and
# hold NaN, so that code reading the pickles finds every key it expects.
RESULT_KEYS_TANGO = ('snr_in_raw', 'sar_cnv', 'sir_cnv', 'sdr_cnv', 'delta_stoi_cnv', 'delta_stoi_dry', 'snr_out', 'snr_in_cnv',
                     'snr_in_dry', 'fw_sd_cnv', 'fw_sd_dry', 'sar_dry', 'sir_dry', 'sdr_dry', 'sdr_in_cnv', 'sir_in_cnv',
                     'sdr_in_dry', 'sir_in_dry', 'sar_in_dry')
RESULT_KEYS_MWF = tuple('delta_stoi' if k == 'delta_stoi_cnv' else k for k in RESULT_KEYS_TANGO)
THIRD_PARTY_KEYS = ('sar_cnv', 'sir_cnv', 'sdr_cnv', 'delta_stoi_cnv', 'delta_stoi', 'delta_stoi_dry', 'sar_dry', 'sir_dry', 'sdr_dry',
                    'sdr_in_cnv', 'sir_in_cnv', 'sdr_in_dry', 'sir_in_dry', 'sar_in_dry')
BSS_KEYS = tuple(k for k in THIRD_PARTY_KEYS if 'stoi' not in k)
STOI_KEYS = tuple(k for k in THIRD_PARTY_KEYS if 'stoi' in k)
# ESTOI (disco_amd.metrics.estoi) is not in the reference's pickles: its keys are added to the two dictionaries only on `estoi=True`, formed
# as their delta_stoi* counterparts; without it the dictionaries, and so the pickles, keep the reference's key set.
ESTOI_KEYS_TANGO = ('delta_estoi_cnv', 'delta_estoi_dry')
ESTOI_KEYS_MWF = ('delta_estoi', 'delta_estoi_dry')
# The segmental SNR (disco_amd.metrics.seg_snr) is not in the reference's pickles either: on `seg_snr=True` both dictionaries gain these two
# keys -- the per-frame level figure the frequency-weighted SNR does not replace -- over windows of SEG_SNR_WINDOW samples of the scored span,
# weighted by vad_oracle_batch of the target image cut to that span.
SEG_SNR_KEYS = ('seg_snr_in_cnv', 'seg_snr_out')
SEG_SNR_WINDOW = (512, 256)             # win_len, win_hop


def room_results(s_in, n_in, sf_t, nf_t, szf_t, nzf_t, rnd_snrs, s_dry=None, n_dry=None, fs=FS, y_in=None, sh_t=None, szh_t=None,
                 bss_flen=512, stoi=False, estoi=False, seg_snr=False):
    """The two result dictionaries of one (room, noise) (tango.py:541-635).
    s_in, n_in (K, L): target / noise images at every node's first microphone; sf_t, nf_t (K, L): their step-2 outputs in time;
    szf_t, nzf_t (K, L): their compressed (step-1) versions in time; rnd_snrs: the drawn input SNRs; s_dry, n_dry (L,): the dry
    sources, or None (the `_dry` metrics are then NaN).  The first second is skipped as in the reference ([fs:]).
    y_in, sh_t, szh_t (K, L): the mixture at every node's first microphone, the step-2 output and the step-1 output in time.  When all
    three are given, the eleven BSS-eval keys (BSS_KEYS) are filled as tango.py:541-567 fills them: references (s_in[k], n_in[k]) for the
    `_cnv` keys and (s_dry, n_dry) for the `_dry` ones; estimates (sh, y - sh) for `res`, (szh, y - szh) for `resz`, (y, y - sh) for the
    `_in_` keys of both; source 0's figures; compute_permutation=False; a `bss_flen`-tap filter (mir_eval's 512).  The differences are
    formed in float64 and rounded to float32 once, which is what the kernels read.  Without them those keys hold NaN.
    stoi=True, with the same three signals: the STOI keys (STOI_KEYS) are filled as tango.py:569-578 fills them -- `delta_stoi_cnv` of `res`
    and `delta_stoi` of `resz` are STOI(s_in[k], sh[k]) and STOI(s_in[k], szh[k]) minus STOI(s_in[k], y[k]); with the dry sources,
    `delta_stoi_dry` of both likewise with s_dry as the clean signal.  All 6 K pairs of the room go in one Engine.stoi call.  The default
    leaves those keys NaN.
    estoi=True: `res` gains `delta_estoi_cnv` and `delta_estoi_dry`, `resz` gains `delta_estoi` and `delta_estoi_dry` (ESTOI_KEYS_TANGO,
    ESTOI_KEYS_MWF), formed as their delta_stoi* counterparts from disco_amd.metrics.estoi on the same pairs; NaN without the three time
    signals (the `_dry` ones without the dry sources).  The default adds no key.
    seg_snr=True: both dictionaries gain `seg_snr_in_cnv` = metrics.seg_snr(s_in, n_in) and `seg_snr_out` -- of (sf_t, nf_t) in `res`, of
    (szf_t, nzf_t) in `resz` (SEG_SNR_KEYS) -- over windows of 512 samples at hop 256 of the scored span [fs:], weighted by
    vad_oracle_batch of the cut s_in.  The default adds no key and no call."""
    from .. import metrics as dm
    K = np.shape(s_in)[0]
    bss = y_in is not None and sh_t is not None and szh_t is not None
    L = min(np.shape(a)[-1] for a in (s_in, n_in, sf_t, nf_t, szf_t, nzf_t) + ((y_in, sh_t, szh_t) if bss else ()) if a is not None)
    if s_dry is not None:
        L = min(L, len(s_dry), len(n_dry))
    cut = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)[..., fs:L])
    nan = np.full(K, np.nan)
    res = {k: nan.copy() for k in RESULT_KEYS_TANGO}
    resz = {k: nan.copy() for k in RESULT_KEYS_MWF}
    res['snr_in_raw'] = resz['snr_in_raw'] = rnd_snrs
    snr_in = np.asarray(dm.fw_snr(cut(s_in), cut(n_in), fs)[1])                        # tango.py:581
    res['snr_in_cnv'] = resz['snr_in_cnv'] = snr_in
    res['snr_out'] = np.asarray(dm.fw_snr(cut(sf_t), cut(nf_t), fs)[1])                # :580
    resz['snr_out'] = np.asarray(dm.fw_snr(cut(szf_t), cut(nzf_t), fs)[1])             # :584
    res['fw_sd_cnv'] = np.asarray(dm.fw_sd(cut(sf_t), cut(s_in), fs)[1])               # :590
    resz['fw_sd_cnv'] = np.asarray(dm.fw_sd(cut(szf_t), cut(s_in), fs)[1])             # :592
    if s_dry is not None:
        sd_, nd_ = cut(s_dry)[None], cut(n_dry)[None]
        dry = float(np.asarray(dm.fw_snr(sd_, nd_, fs)[1]).reshape(-1)[0])
        res['snr_in_dry'] = resz['snr_in_dry'] = np.full(K, dry)                       # :582, 586
        rep = np.repeat(sd_, K, axis=0)
        res['fw_sd_dry'] = np.asarray(dm.fw_sd(cut(sf_t), rep, fs)[1])                 # :591
        resz['fw_sd_dry'] = np.asarray(dm.fw_sd(cut(szf_t), rep, fs)[1])               # :593
    if bss:
        cut64 = lambda a: np.asarray(a, dtype=np.float32)[..., fs:L].astype(np.float64)
        y, sh, szh = cut64(y_in), cut64(sh_t), cut64(szh_t)
        f32 = lambda a: a.astype(np.float32)
        # (K, 3, 2, L'): ests (:547), ests_z (:548), ests_i (:549) of every node
        ests = np.stack([np.stack([f32(sh), f32(y - sh)], 1), np.stack([f32(szh), f32(y - szh)], 1), np.stack([f32(y), f32(y - sh)], 1)], 1)

        def figures(refs, est):
            """refs (n_set, 2, L'), est (n_set, n_est, 2, L') -> sdr, sir, sar of source 0, each (n_set, n_est)."""
            en, status = dm._engine().bss_eval(refs, est, flen=bss_flen)
            dm._raise_on_zero_reference(refs, status)
            return tuple(v[..., 0] for v in dm._figures(en))

        sdr, sir, sar = figures(np.stack([cut(s_in), cut(n_in)], 1), ests)                 # :562-564
        res['sdr_cnv'], res['sir_cnv'], res['sar_cnv'] = sdr[:, 0], sir[:, 0], sar[:, 0]
        resz['sdr_cnv'], resz['sir_cnv'], resz['sar_cnv'] = sdr[:, 1], sir[:, 1], sar[:, 1]
        res['sdr_in_cnv'] = resz['sdr_in_cnv'] = sdr[:, 2]                                 # :567
        res['sir_in_cnv'] = resz['sir_in_cnv'] = sir[:, 2]
        if s_dry is not None:                                                              # :552-560: one reference set, 3 K estimate sets
            sdr, sir, sar = (v.reshape(K, 3) for v in figures(np.stack([cut(s_dry), cut(n_dry)], 0)[None], ests.reshape(1, 3 * K, 2, -1)))
            res['sdr_dry'], res['sir_dry'], res['sar_dry'] = sdr[:, 0], sir[:, 0], sar[:, 0]
            resz['sdr_dry'], resz['sir_dry'], resz['sar_dry'] = sdr[:, 1], sir[:, 1], sar[:, 1]
            res['sdr_in_dry'] = resz['sdr_in_dry'] = sdr[:, 2]
            res['sir_in_dry'] = resz['sir_in_dry'] = sir[:, 2]
            res['sar_in_dry'] = resz['sar_in_dry'] = sar[:, 2]
    if estoi:
        for r, keys in ((res, ESTOI_KEYS_TANGO), (resz, ESTOI_KEYS_MWF)):
            r.update({k: nan.copy() for k in keys})
    if seg_snr:
        from .. import sigproc_utils as su
        vad = su.vad_oracle_batch(cut(s_in))
        seg = lambda s, n: np.asarray(dm.seg_snr(cut(s), cut(n), *SEG_SNR_WINDOW, vad=vad))
        res['seg_snr_in_cnv'] = resz['seg_snr_in_cnv'] = seg(s_in, n_in)
        res['seg_snr_out'], resz['seg_snr_out'] = seg(sf_t, nf_t), seg(szf_t, nzf_t)
    measures = [(nm, f) for nm, f, on in (('stoi', dm.stoi, stoi), ('estoi', dm.estoi, estoi)) if on and bss]
    if measures:                                                                           # the pairs are stacked once for both measures
        clean = [cut(s_in)] + ([np.repeat(cut(s_dry)[None], K, axis=0)] if s_dry is not None else [])
        proc = np.stack([cut(y_in), cut(sh_t), cut(szh_t)])                                # (3, K, L'): in, out, out_z
        x = np.stack([np.broadcast_to(c, proc.shape) for c in clean])                      # (1 or 2, 3, K, L')
    for name, measure in measures:
        d = np.asarray(measure(x, np.broadcast_to(proc, x.shape), fs))                     # tango.py:569-574
        res[f'delta_{name}_cnv'] = d[0, 1] - d[0, 0]                                       # :575
        resz[f'delta_{name}'] = d[0, 2] - d[0, 0]                                          # :577
        if s_dry is not None:
            res[f'delta_{name}_dry'] = d[1, 1] - d[1, 0]                                   # :576
            resz[f'delta_{name}_dry'] = d[1, 2] - d[1, 0]                                  # :578
    return res, resz


# ---- a whole batch of rooms in one call -----------------------------------------------------------------------------------------
def _is_host(a):
    return isinstance(a, np.ndarray) or not hasattr(a, 'data_ptr')


def _batch_array(a, lead, name):
    """NumPy -> contiguous float32; a device-resident torch tensor stays where it is.  Leading axes checked."""
    if _is_host(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
    elif not a.is_contiguous():
        raise ValueError(f'{name}: device tensors must be contiguous')
    if tuple(int(v) for v in a.shape[:-1]) != tuple(lead):
        raise ValueError(f'{name}: expected leading axes {tuple(lead)}, got shape {tuple(a.shape)}')
    return a


def _xp(arrays):
    """numpy, or torch when every array is a device tensor (the stacking below then happens on the device)."""
    host = [_is_host(a) for a in arrays]
    if all(host):
        return np, True
    if any(host):
        raise TypeError('batch_results: pass every signal as a NumPy array or every signal as a device-resident torch tensor')
    import torch
    return torch, False


def _trim(a, L):
    return a if int(a.shape[-1]) == L else a[..., :L]


def batch_results(s_in, n_in, sf_t, nf_t, szf_t, nzf_t, rnd_snrs, s_dry=None, n_dry=None, fs=FS, y_in=None, sh_t=None, szh_t=None,
                  bss_flen=512, stoi=False, lengths=None, estoi=False, seg_snr=False):
    """`room_results` for a whole batch of rooms, clips of different lengths included, in a handful of launches instead of one pass of
    Python per room: signals (R, K, L), dry sources (R, L), rnd_snrs (R, ...), as NumPy arrays (copied to the device) or -- all of them --
    device-resident torch tensors (read in place; no signal comes to the host).  lengths (R,): room r is scored over [fs, lengths[r]),
    the reference's [fs : min_len]; None: the smallest last axis among the signals, for every room, as `room_results` takes it.
    Samples at and beyond lengths[r] are never read and may hold anything, NaN included.
    Returns (res, resz) with the keys of `room_results`, every value (R, K) (`snr_in_raw` is rnd_snrs as given); row r holds what
    `room_results` returns for room r alone on signals cut to lengths[r] (`results_of_room` takes it out).
    The band levels of a dry source are computed once per room.  The BSS part walks whole rooms in chunks whose workspace stays under
    Engine.BSS_WORKSPACE_BUDGET: a chunk's estimate sets are formed on the device (Engine.bss_estimates, 24 L bytes per node) and scored
    twice, against (s_in, n_in) per node and against the room's dry pair with 3 K estimate sets.  An all-zero reference raises
    ValueError naming the room and the node.  STOI: one Engine.stoi call for all 6 R K pairs, with a stop per pair; estoi=True: the
    four ESTOI keys of `room_results` from one Engine.estoi call on the same pairs and stops.  seg_snr=True: the two segmental-SNR keys of
    `room_results` (SEG_SNR_KEYS) in both dictionaries, from one Engine.vad_samples and three Engine.seg_snr calls on the signals cut to
    [fs:], with a stop per (room, node)."""
    from .. import metrics as dm
    R, K = (int(v) for v in np.shape(s_in)[:2])
    bss = y_in is not None and sh_t is not None and szh_t is not None
    dry = s_dry is not None
    names = ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t') + (('y_in', 'sh_t', 'szh_t') if bss else ())
    given = (s_in, n_in, sf_t, nf_t, szf_t, nzf_t) + ((y_in, sh_t, szh_t) if bss else ())
    sig = {nm: _batch_array(a, (R, K), nm) for nm, a in zip(names, given)}
    if dry:
        sig['s_dry'], sig['n_dry'] = _batch_array(s_dry, (R,), 's_dry'), _batch_array(n_dry, (R,), 'n_dry')
    xp, host = _xp(list(sig.values()))
    Lmin = min(int(a.shape[-1]) for a in sig.values())
    fs = int(fs)
    if lengths is None:
        lens = np.full((R,), Lmin, dtype=np.int64)
    else:
        lens = np.asarray(lengths)
        if lens.shape != (R,) or not np.issubdtype(lens.dtype, np.integer):
            raise ValueError(f'lengths must hold one integer per room, shape ({R},): got {lens.dtype} {lens.shape}')
        if np.any(lens < fs) or np.any(lens > Lmin):
            raise ValueError(f'need fs = {fs} <= lengths <= {Lmin}, the shortest signal: {lens}')
        lens = lens.astype(np.int64)
    stop_rk = np.repeat(lens, K)                                                          # one stop per (room, node)
    eng = dm._engine()
    F, I = dm.band_importance(fs)
    fb, fa = dm.third_octave_filterbank(F, fs, order=4)

    def levels(nm):
        """band levels of every signal of `nm` over its own room's span: (R, K, n_bands), or (R, n_bands) for a dry source"""
        a = sig[nm]
        lead = tuple(int(v) for v in a.shape[:-1])
        st = eng.band_stats(a.reshape(-1, int(a.shape[-1])), fb, fa, fs, stop_rk if len(lead) == 2 else lens).numpy()
        return dm._var_nz(st[..., 0], st[..., 1], st[..., 2]).reshape(lead + (fb.shape[0],))

    nan = np.full((R, K), np.nan)
    res = {k: nan.copy() for k in RESULT_KEYS_TANGO}
    resz = {k: nan.copy() for k in RESULT_KEYS_MWF}
    res['snr_in_raw'] = resz['snr_in_raw'] = rnd_snrs
    lv = {nm: levels(nm) for nm in ('s_in', 'n_in', 'sf_t', 'nf_t', 'szf_t', 'nzf_t')}
    fw_snr = lambda num, den: dm._weighted_band_db(num, den, I, -15)[1]
    fw_sd = lambda out, ref: dm._weighted_band_db(ref, out, I, 0)[1]
    res['snr_in_cnv'] = resz['snr_in_cnv'] = fw_snr(lv['s_in'], lv['n_in'])              # tango.py:581
    res['snr_out'] = fw_snr(lv['sf_t'], lv['nf_t'])                                       # :580
    resz['snr_out'] = fw_snr(lv['szf_t'], lv['nzf_t'])                                    # :584
    res['fw_sd_cnv'] = fw_sd(lv['sf_t'], lv['s_in'])                                      # :590
    resz['fw_sd_cnv'] = fw_sd(lv['szf_t'], lv['s_in'])                                    # :592
    if dry:
        lsd, lnd = levels('s_dry'), levels('n_dry')                                       # (R, n_bands): once per room
        res['snr_in_dry'] = resz['snr_in_dry'] = np.repeat(fw_snr(lsd, lnd)[:, None], K, axis=1)      # :582, 586
        res['fw_sd_dry'] = fw_sd(lv['sf_t'], lsd[:, None, :])                             # :591
        resz['fw_sd_dry'] = fw_sd(lv['szf_t'], lsd[:, None, :])                           # :593
    if bss:
        Lb = min(int(sig[nm].shape[-1]) for nm in ('y_in', 'sh_t', 'szh_t'))
        y, sh, szh = (_trim(sig[nm], Lb) for nm in ('y_in', 'sh_t', 'szh_t'))
        Lr = min(Lb, int(sig['s_in'].shape[-1]), int(sig['n_in'].shape[-1]))
        if dry:
            Lr = min(Lr, int(sig['s_dry'].shape[-1]), int(sig['n_dry'].shape[-1]))
        flen = int(bss_flen)
        per_set = int(eng.lib.disco_bss_workspace_bytes(eng.ctx, 1, 2, flen, Lr))
        rooms = R if per_set == 0 else max(1, min(R, eng.BSS_WORKSPACE_BUDGET // (per_set * K)))     # per_set 0: bss_eval names the limit
        cont = (lambda a: np.ascontiguousarray(a)) if host else (lambda a: a.contiguous())

        def figures(refs, est, stops, r0, per_node):
            """refs (n_set, 2, L), est (n_set, n_est, 2, L) -> sdr, sir, sar of source 0, each (n_set, n_est)"""
            en, status = eng.bss_eval(refs, est, fs, stops, flen)
            if np.any(status != 0):
                n_set = int(refs.shape[0])
                r2 = refs.reshape(2 * n_set, Lr)
                e_ref = eng.pair_stats(r2, r2, fs, np.repeat(stops, 2)).numpy()[:, 2]
                zero = np.flatnonzero(e_ref == 0)
                if zero.size:
                    i, j = int(zero[0]) // 2, int(zero[0]) % 2
                    where = f'room {r0 + i // K}, node {i % K}' if per_node else f'room {r0 + i}, every node (dry sources)'
                    raise ValueError(f'{where}: reference source {j} is all zero over the scored span')
            return tuple(v[..., 0] for v in dm._figures(en))

        out = {k: np.empty((R, K, 3)) for k in ('sdr', 'sir', 'sar', 'sdr_dry', 'sir_dry', 'sar_dry')}
        for r0 in range(0, R, rooms):
            r1 = min(R, r0 + rooms)
            n = r1 - r0
            # (n K, 3, 2, Lr): ests (:547), ests_z (:548), ests_i (:549) of every node of the chunk's rooms
            ests = eng.bss_estimates(*(cont(_trim(a[r0:r1], Lr)).reshape(n * K, Lr) for a in (y, sh, szh)), start=fs, stop=stop_rk[r0 * K:r1 * K])
            refs = xp.stack([_trim(sig['s_in'][r0:r1], Lr), _trim(sig['n_in'][r0:r1], Lr)], 2).reshape(n * K, 2, Lr)
            for key, v in zip(('sdr', 'sir', 'sar'), figures(refs, ests, stop_rk[r0 * K:r1 * K], r0, True)):      # :562-567
                out[key][r0:r1] = v.reshape(n, K, 3)
            if dry:                                                                       # :552-560: one reference set, 3 K estimate sets
                refs = xp.stack([_trim(sig['s_dry'][r0:r1], Lr), _trim(sig['n_dry'][r0:r1], Lr)], 1)
                for key, v in zip(('sdr_dry', 'sir_dry', 'sar_dry'), figures(refs, ests.reshape(n, 3 * K, 2, Lr), lens[r0:r1], r0, False)):
                    out[key][r0:r1] = v.reshape(n, K, 3)
            del ests
        sdr, sir, sar = out['sdr'], out['sir'], out['sar']
        res['sdr_cnv'], res['sir_cnv'], res['sar_cnv'] = sdr[..., 0], sir[..., 0], sar[..., 0]
        resz['sdr_cnv'], resz['sir_cnv'], resz['sar_cnv'] = sdr[..., 1], sir[..., 1], sar[..., 1]
        res['sdr_in_cnv'] = resz['sdr_in_cnv'] = sdr[..., 2]
        res['sir_in_cnv'] = resz['sir_in_cnv'] = sir[..., 2]
        if dry:
            sdr, sir, sar = out['sdr_dry'], out['sir_dry'], out['sar_dry']
            res['sdr_dry'], res['sir_dry'], res['sar_dry'] = sdr[..., 0], sir[..., 0], sar[..., 0]
            resz['sdr_dry'], resz['sir_dry'], resz['sar_dry'] = sdr[..., 1], sir[..., 1], sar[..., 1]
            res['sdr_in_dry'] = resz['sdr_in_dry'] = sdr[..., 2]
            res['sir_in_dry'] = resz['sir_in_dry'] = sir[..., 2]
            res['sar_in_dry'] = resz['sar_in_dry'] = sar[..., 2]
    if estoi:
        for r, keys in ((res, ESTOI_KEYS_TANGO), (resz, ESTOI_KEYS_MWF)):
            r.update({k: nan.copy() for k in keys})
    if seg_snr:
        cut = lambda a: (np.ascontiguousarray(a[..., fs:Lmin]) if host else a[..., fs:Lmin].contiguous()).reshape(R * K, Lmin - fs)
        stops = (stop_rk - fs).astype(np.int32)
        vad = eng.vad_samples(cut(sig['s_in']), stop=stops)

        def seg(s, n):
            st = eng.seg_snr(cut(sig[s]), cut(sig[n]), *SEG_SNR_WINDOW, vad=vad, stop=stops).numpy()
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.where(st[:, 2] > 0, st[:, 0] / st[:, 1], np.nan).reshape(R, K)

        res['seg_snr_in_cnv'] = resz['seg_snr_in_cnv'] = seg('s_in', 'n_in')
        res['seg_snr_out'], resz['seg_snr_out'] = seg('sf_t', 'nf_t'), seg('szf_t', 'nzf_t')
    measures = [(nm, f) for nm, f, on in (('stoi', eng.stoi, stoi), ('estoi', eng.estoi, estoi)) if on and bss]
    if measures:                                                                          # the pairs are stacked once for both measures
        Ls = Lr
        flat = lambda a: _trim(a, Ls).reshape(R * K, Ls)
        clean = [flat(sig['s_in'])]
        if dry:
            d2 = _trim(sig['s_dry'], Ls)
            clean.append((np.repeat(d2, K, axis=0) if host else d2.repeat_interleave(K, dim=0)))
        cat = (lambda parts: np.concatenate(parts, 0)) if host else (lambda parts: xp.cat(parts, 0))
        proc = [flat(sig[nm]) for nm in ('y_in', 'sh_t', 'szh_t')]                        # in, out, out_z
        x = cat([c for c in clean for _ in proc])                                         # (6 R K or 3 R K, Ls): [clean][proc][room][node]
        yy = cat([p for _ in clean for p in proc])
    for name, measure in measures:
        d, status = measure(x, yy, fs, fs, np.tile(stop_rk, len(clean) * 3))              # tango.py:569-574
        if np.any(status == 2):
            i = int(np.flatnonzero(status == 2)[0]) % (R * K)
            raise ValueError(f'room {i // K}, node {i % K}: the scored span is too short for one frame (fewer than 257 samples at 10 kHz)')
        if np.any(status == 1):
            import warnings
            warnings.warn('Not enough STFT frames to compute intermediate intelligibility measure after removing silent frames. '
                          'Returning 1e-5. Please check you wav files', RuntimeWarning)
        d = d.reshape(len(clean), 3, R, K)
        res[f'delta_{name}_cnv'] = d[0, 1] - d[0, 0]                                      # :575
        resz[f'delta_{name}'] = d[0, 2] - d[0, 0]                                         # :577
        if dry:
            res[f'delta_{name}_dry'] = d[1, 1] - d[1, 0]                                  # :576
            resz[f'delta_{name}_dry'] = d[1, 2] - d[1, 0]                                 # :578
    return res, resz


def results_of_room(res, resz, r):
    """Room r of `batch_results`' two dictionaries: the two per-room dictionaries `room_results` returns and `write_result_pickles` takes."""
    return {k: np.asarray(v)[r] for k, v in res.items()}, {k: np.asarray(v)[r] for k, v in resz.items()}


def write_result_pickles(root, i_rir, noise, res, resz):
    """<root>/OIM/results_tango_<i_rir>_<noise>.p and results_mwf_... (tango.py:634-635)."""
    import pickle
    d = os.path.join(root, 'OIM')
    os.makedirs(d, exist_ok=True)
    files = []
    for name, r in (('tango', res), ('mwf', resz)):
        p = os.path.join(d, 'results_{}_{}_{}.p'.format(name, i_rir, noise))
        with open(p, 'wb') as f:
            pickle.dump(r, f)
        files.append(p)
    return files
