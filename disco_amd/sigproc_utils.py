"""`tf_mask`, `vad_oracle_batch` and `increase_to_snr` with the reference's names and argument order (disco_theque/sigproc_utils.py:58-86
== dnn/utils.py:44-71, :12-55, :194-224).  The last two follow the conventions of disco_amd.metrics: the last axis is time, the leading axes a
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
