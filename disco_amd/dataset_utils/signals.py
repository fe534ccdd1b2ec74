"""target_segments, noise_segments, ssn_segments: the dry sources simulate_rooms starts from, prepared on the device.

    target_segments   signal_setups.py:42-73     trim, de-mean, VAD, level the voiced variance to var_tar, VAD again, 1 s of silence in front
    noise_segments    signal_setups.py:133-136   a file segment wrapped from a start, cut, de-meaned
    ssn_segments      signal_setups.py:95-98     speech-shaped noise: noise_from_signal of the stacked talkers, cut

The signals stay on the device (DevBuf); only moments (sums, variances) and flags come to the host.  Nothing is read from files and nothing
is drawn here except the phases of ssn_segments when none are given: which file, which start, which talkers stay the caller's job.
"""
import numpy as np

from .. import sigproc_utils as su
from .._engines import get_engine
from ..engine import DevBuf


def _engine():
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)      # these kernels do not depend on the batch geometry


def _dev(eng, a):
    """A float32 array on the device as it is, a NumPy array uploaded: -> something Engine methods answer with a DevBuf for."""
    if isinstance(a, DevBuf) or hasattr(a, 'data_ptr'):
        return a
    return eng.to_device(np.ascontiguousarray(a, dtype=np.float32), np.float32)[1]


def _rows(signals, lengths, what):
    """(device array (R, L), R, L, lengths (R,) int64 checked against L)."""
    eng = _engine()
    signals = _dev(eng, signals)
    if len(signals.shape) != 2:
        raise ValueError(f'{what} must be (R, L): {tuple(signals.shape)}')
    R, L = (int(v) for v in signals.shape)
    lens = np.asarray(lengths)
    if not np.issubdtype(lens.dtype, np.integer):
        raise ValueError(f'lengths must hold integers, got {lens.dtype}')
    try:
        lens = np.broadcast_to(lens, (R,)).astype(np.int64)
    except ValueError:
        raise ValueError(f'lengths of shape {np.shape(lengths)} is not one value per signal ({R})') from None
    if np.any(lens < 0) or np.any(lens > L):
        raise ValueError(f'need 0 <= lengths <= L = {L}: {lengths}')
    return eng, signals, R, L, lens


def _means(eng, x, stops):
    """The float64 mean of x[i, :stops[i]] from the device's float64 sums (Engine.pair_stats); 0 for an empty row."""
    st = eng.pair_stats(x, x, 0, stops.astype(np.int32)).numpy()
    return np.where(stops > 0, st[:, 1] / np.maximum(stops, 1), 0.0)


def target_segments(signals, lengths, var_tar, duration_range, fs=16000):
    """get_target_segment (signal_setups.py:42-73) for R signals: signals (R, L) float32 with lengths (R,) valid samples each,
    duration_range = (min_duration, max_duration) in seconds.
      1. the signal is trimmed to int(max_duration * fs) samples, 2. the mean over the trimmed signal is removed,
      3. vad_oracle_batch(thr=0.001) of it, 4. gain = sqrt(var_tar / var(signal[vad == 1])), 5. the VAD of the scaled signal,
      6. fs zeros are put in front of both.
    -> dict.  On the device: signal, vad (R, fs + Lmax), Lmax the longest trimmed length.  NumPy: lengths (R,) (fs + the trimmed length),
    duration (R,) (the reference's target_duration: trimmed length / fs + 1), gain (R,), ok (R,) bool.
    ok is False where the signal is shorter than min_duration (the reference returns None) or has no voiced sample (the reference divides
    by the variance of nothing); such rows are zeros in signal and vad, their lengths and gain 0.  Both go to simulate_rooms as they are."""
    eng, x, R, L, lens = _rows(signals, lengths, 'signals')
    min_duration, max_duration = float(duration_range[0]), float(duration_range[1])
    fs = int(fs)
    trimmed = np.minimum(lens, int(max_duration * fs))
    Lmax = int(trimmed.max(initial=0))
    stops = trimmed.astype(np.int32)
    long_enough = trimmed / fs >= min_duration
    mean = _means(eng, x, trimmed)
    centred = eng.affine_segment(x, stop=stops, mean=mean, out_len=Lmax)
    with np.errstate(divide='ignore', invalid='ignore'):                        # a row without a voiced sample: 0 / 0, flagged below
        var = np.asarray(su._gated_var(centred, su.vad_oracle_batch(centred, thr=0.001, stop=stops), stops), np.float64).reshape(R)
        gain = np.sqrt(var_tar / var)
    ok = long_enough & np.isfinite(gain) & (gain > 0)
    gain = np.where(ok, gain, 0.0)
    count = np.where(ok, trimmed, 0).astype(np.int32)                           # count 0: an all-zero row
    signal = eng.affine_segment(x, stop=stops, count=count, mean=mean, gain=gain, lead=fs, out_len=fs + Lmax)
    # the VAD sees the scaled signal without its leading silence (the threshold is a quantile of the signal's own samples)
    scaled = eng.affine_segment(x, stop=stops, count=count, mean=mean, gain=gain, out_len=Lmax)
    vad = eng.affine_segment(su.vad_oracle_batch(scaled, thr=0.001, stop=count), stop=count, lead=fs, out_len=fs + Lmax)
    return dict(signal=signal, vad=vad, lengths=np.where(ok, fs + trimmed, 0), duration=trimmed / fs + 1, gain=gain, ok=ok)


def noise_segments(noise, lengths, start, duration, fs=16000):
    """_read_random_signal's last lines (signal_setups.py:133-136) for R files: noise (R, L) float32 with lengths (R,) valid samples,
    start (R,) the sample each cut starts at (the reference's rnd_start), duration in seconds (a scalar).
        y = np.roll(sig, len(sig) - start)[:int(duration * fs)];  y -= np.mean(y)
    -> (R, n) on the device, n = int(duration * fs).  A file shorter than the cut gives its own length (the reference's slice), the rest
    of the row zeros.  The mean is that of the cut, from float64 sums on the device."""
    eng, x, R, L, lens = _rows(noise, lengths, 'noise')
    n = int(duration * int(fs))
    if n < 0:
        raise ValueError(f'duration must not be negative: {duration}')
    start = np.asarray(start)
    if not np.issubdtype(start.dtype, np.integer):
        raise ValueError(f'start must hold integers, got {start.dtype}')
    start = np.broadcast_to(start, (R,)).astype(np.int32)
    stops, count = lens.astype(np.int32), np.minimum(lens, n).astype(np.int32)
    cut = eng.affine_segment(x, stop=stops, start=start, count=count, out_len=n)
    return eng.affine_segment(cut, stop=count, mean=_means(eng, cut, count.astype(np.int64)), out_len=n)


def ssn_segments(talkers, lengths, duration, fs=16000, phase=None):
    """The 'SSN' branch of get_noise_segment (signal_setups.py:95-98) for R rows of stacked talkers: talkers (R, L) float32 with lengths
    (R,) valid samples each -> noise_from_signal(talkers_i[:lengths_i])[:int(duration * fs)], (R, n) on the device with
    n = min(int(duration * fs), L).  phase: as disco_amd.sigproc_utils.noise_from_signal takes it (None: drawn from NumPy's global
    generator row by row).  513 <= lengths <= 2^22."""
    eng, x, R, L, lens = _rows(talkers, lengths, 'talkers')
    n = min(int(duration * int(fs)), L)
    if n < 0:
        raise ValueError(f'duration must not be negative: {duration}')
    full = su.noise_from_signal(x, stop=lens.astype(np.int32), phase=phase)
    return eng.affine_segment(full, stop=np.minimum(lens, n).astype(np.int32), out_len=n)
