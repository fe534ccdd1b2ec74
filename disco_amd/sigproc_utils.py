"""`tf_mask`, `vad_oracle_batch`, `increase_to_snr` and `noise_from_signal` with the reference's names and argument order
(disco_theque/sigproc_utils.py:58-86 == dnn/utils.py:44-71, :12-55, :194-224, :257-279).  The last three follow the conventions of disco_amd.metrics: the last axis is time, the leading axes a
batch, NumPy in gives NumPy out, a device array (torch tensor or DevBuf) in gives a DevBuf out, `stop` is None, a scalar or an array broadcast
over the leading axes."""
import numpy as np

from ._engines import get_engine
from .engine import parse_mask_type

_IDENTITY_BAND = np.eye(1, 9)            # b = a = [1, 0, ..., 0]: the "band" whose output is the signal itself


def _engine():
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)      # these kernels do not depend on the batch geometry


def vad_oracle_batch(x_, win_len=512, win_hop=256, thr=0.001, rat=2, stop=None):
    """sigproc_utils.py:12-55 for a batch: x_ (..., L) -> the per-sample VAD (..., L), float32 0 / 1 (Engine.vad_samples).  Signal i is
    processed as if sliced to stop[i] and run alone; its VAD is zero at and beyond stop[i]."""
    return _engine().vad_samples(x_, stop=stop, win_len=win_len, win_hop=win_hop, thr=thr, rat=rat)


def _gated_var(x, vad, stop):
    """np.var of the samples where the VAD is non-zero (of the non-zero samples without one), per leading index: the gated band statistics
    with the identity band -- the float64 count, sum and sum of squares behind fw_snr's levels, no kernel of its own."""
    from . import metrics
    return metrics._band_levels(x, _IDENTITY_BAND, _IDENTITY_BAND, 0, stop, gate=vad)[..., 0]


def snr_gain(x, n, snr_out, vad_tar=None, vad_noi=None, weight=False, fs=None, stop=None):
    """The factor increase_to_snr multiplies the noise by, one float64 per leading index (sigproc_utils.py:210-223); only moments of the
    signals come to the host.  snr_out: a scalar or one value per leading index."""
    from . import metrics
    if weight:
        snr_0 = metrics.fw_snr(x, n, fs, vad_tar=vad_tar, vad_noi=vad_noi, stop=stop)[1]
        return 10 ** ((snr_0 - np.asarray(snr_out, np.float64)) / 20)
    var_x, var_n = _gated_var(x, vad_tar, stop), _gated_var(n, vad_noi, stop)
    return np.sqrt(10 ** (-np.asarray(snr_out, np.float64) / 10) * var_x / var_n)


def increase_to_snr(x, n, snr_out, vad_tar=None, vad_noi=None, weight=False, fs=None, stop=None, return_gain=False):
    """sigproc_utils.py:194-224, batched: the noise n (..., L) scaled so that the SNR between x and it is snr_out -- the mean of
    metrics.fw_snr with weight=True, else the ratio of the variances over the samples where the VADs are non-zero (the non-zero samples
    without a VAD).  The signals are scaled on the device (Engine.mix_scaled): zeros at and beyond stop.  return_gain: -> (n_, gain)."""
    gain = snr_gain(x, n, snr_out, vad_tar, vad_noi, weight, fs, stop)
    lead = tuple(int(v) for v in n.shape[:-1]) if hasattr(n, 'shape') else np.shape(n)[:-1]
    try:
        g = np.broadcast_to(gain, lead)
    except ValueError:
        raise ValueError(f'snr_out of shape {np.shape(snr_out)} does not broadcast to the leading axes {lead}') from None
    n_ = _engine().mix_scaled(None, n, g.reshape(-1), group=1, stop=stop, want_y=False)[0]
    return (n_, np.array(g)) if return_gain else n_


NOISE_MIN_LEN, NOISE_MAX_LEN = 513, 1 << 22      # signals disco_noise_from_signal transforms: n_fft = 2^10 ... 2^22


def noise_from_signal(x, stop=None, phase=None):
    """sigproc_utils.py:257-279 for a batch: x (..., L) -> noise (..., L) with the magnitude spectrum of each signal and random phases
    (Engine.noise_from_signal).  Signal i is processed as if sliced to L_i = stop[i] and run alone, with n_fft_i = next_pow_2(L_i); zeros at
    and beyond L_i.  Rows are grouped by n_fft, one launch group each (a device array: runs of consecutive rows of one n_fft).
    phase=None draws np.random.random(n_fft_i / 2 + 1) row by row from NumPy's global generator: one signal under a seed gets the
    reference's own phases.  Otherwise phase is an array in turns, [0, 1): on the host (..., F) with F >= n_fft_i / 2 + 1 for every row,
    row i taking its first n_fft_i / 2 + 1 values; on the device (..., n_fft / 2 + 1), every row then sharing one n_fft.
    513 <= L_i <= 2^22, else ValueError."""
    from .engine import DevBuf, Engine, _on_host
    from .math_utils import next_pow_2
    host = _on_host(x)
    if host:
        x = np.ascontiguousarray(x, dtype=np.float32)
    shape = tuple(int(v) for v in x.shape)
    lead, L = shape[:-1], shape[-1]
    n_sig = int(np.prod(lead, dtype=np.int64))
    stops = Engine._lead_stops(stop, lead, L)
    lens = np.full(n_sig, L, np.int64) if stops is None else stops.astype(np.int64)
    if n_sig and (lens.min() < NOISE_MIN_LEN or lens.max() > NOISE_MAX_LEN):
        raise ValueError(f'noise_from_signal takes signals of {NOISE_MIN_LEN} to {NOISE_MAX_LEN} = 2^22 samples (n_fft = 2^10 ... 2^22): '
                         f'got lengths from {int(lens.min())} to {int(lens.max())}')
    n_ffts = np.array([next_pow_2(int(v)) for v in lens], np.int64)
    if phase is None:
        drawn = [np.random.random(int(n) // 2 + 1) for n in n_ffts]
        phase_of = lambda rows, n_fft: np.stack([drawn[r] for r in rows]).astype(np.float32)
    elif _on_host(phase):
        ph = np.asarray(phase, np.float32)
        if ph.shape[:-1] != lead or (n_sig and ph.shape[-1] < int(n_ffts.max()) // 2 + 1):
            raise ValueError(f'phase must be {lead} + (F,), F >= n_fft / 2 + 1 = {int(n_ffts.max()) // 2 + 1}: {ph.shape}')
        ph = ph.reshape(n_sig, -1)
        phase_of = lambda rows, n_fft: np.ascontiguousarray(ph[rows, :n_fft // 2 + 1])
    else:
        if len(set(n_ffts.tolist())) > 1 or tuple(int(v) for v in phase.shape) != lead + (int(n_ffts[0]) // 2 + 1,):
            raise ValueError('a device phase must be (..., n_fft / 2 + 1) with one n_fft for every row')
        phase_of = lambda rows, n_fft: phase
    eng = _engine()
    if host:
        x2 = x.reshape(n_sig, L)
        out = np.zeros((n_sig, L), np.float32)
        for n_fft in sorted(set(n_ffts.tolist())):
            rows = np.flatnonzero(n_ffts == n_fft)
            out[rows] = eng.noise_from_signal(x2[rows], phase_of(rows, n_fft), stop=None if stops is None else stops[rows], n_fft=n_fft)
        return out.reshape(shape)
    out = eng.empty(shape, np.float32)
    flat = lambda a, r0, r1, w: a.part(r0 * w, (r1 - r0, w)) if isinstance(a, DevBuf) else a.reshape(n_sig, w)[r0:r1]
    r0 = 0
    while r0 < n_sig:                                       # runs of consecutive rows with one n_fft
        r1 = r0 + 1
        while r1 < n_sig and n_ffts[r1] == n_ffts[r0]:
            r1 += 1
        n_fft, rows = int(n_ffts[r0]), np.arange(r0, r1)
        p = phase_of(rows, n_fft)
        eng.noise_from_signal(flat(x, r0, r1, L), p if _on_host(p) else flat(p, r0, r1, n_fft // 2 + 1),
                              stop=None if stops is None else stops[r0:r1], n_fft=n_fft, out=out.part(r0 * L, (r1 - r0, L)))
        r0 = r1
    return out


def tf_mask(s, n, type='irm1', bin_thr=0):
    """Oracle TF mask from target / noise STFTs.  Raises ValueError for an unknown type (dnn/utils.py:69) and
    AssertionError on a shape mismatch (sigproc_utils.py:71), like the reference."""
    parse_mask_type(type)                                  # ValueError before touching the device
    s = np.asarray(s)
    n = np.asarray(n)
    assert s.shape == n.shape, 'Target and noise STFTs should have the same shape'
    eng = get_engine(rooms=1, nodes=1, mics=1, length=1024)
    m = eng.tf_mask(np.ascontiguousarray(s, dtype=np.complex64), np.ascontiguousarray(n, dtype=np.complex64),
                    type=type, bin_thr=float(bin_thr)).numpy()
    return m.astype(bool) if type.startswith('ibm') else m
