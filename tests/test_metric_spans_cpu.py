"""Host-only logic of the per-signal spans (no GPU, no emulator): how a `stop` array is broadcast over the leading axes in disco_amd.metrics,
what Engine's metric methods accept as `stop`, the arithmetic fw_snr and fw_sd share with results_io.batch_results, and the argument
errors of batch_results / results_of_room."""
import numpy as np
import pytest

from disco_amd import metrics as dm
from disco_amd.engine import Engine
from disco_amd.speech_enhancement import results_io as rio
from oracle import metrics_oracle as meo


def test_stop_broadcasts_over_the_leading_axes():
    assert dm._span_stops(None, (3, 2)) is None and dm._span_stops(7, (3, 2)) == 7 and dm._span_stops(np.int64(7), ()) == 7
    full = np.arange(6).reshape(3, 2)
    assert np.array_equal(dm._span_stops(full, (3, 2)), np.arange(6))
    assert np.array_equal(dm._span_stops(np.array([[5], [6], [7]]), (3, 2)), [5, 5, 6, 6, 7, 7])        # one stop per room, K nodes
    assert np.array_equal(dm._span_stops([8, 9], (3, 2)), [8, 9, 8, 9, 8, 9])
    assert dm._span_stops(full, (3, 2)).flags['C_CONTIGUOUS']
    with pytest.raises(ValueError, match='does not broadcast to the leading axes'):
        dm._span_stops(np.arange(3), (3, 2))


class _Uploaded(Exception):
    pass


def _bare_engine(uploads):
    eng = Engine.__new__(Engine)                  # no library, no context: only the host-side argument handling is exercised
    eng.ctx = None

    def to_device(a, dtype):
        uploads.append((np.array(a), np.dtype(dtype)))
        return 1234, a
    eng.to_device = to_device
    return eng


def test_engine_stop_none_scalar_or_one_per_signal():
    ups = []
    eng = _bare_engine(ups)
    assert eng._span_stops(None, 4, 100, 10) == (100, None) and eng._span_stops(np.int32(60), 4, 100, 10) == (60, None) and not ups
    stop, dev = eng._span_stops(np.array([10, 50, 100, 99], np.int64), 4, 100, 10)
    assert stop is None and dev[0] == 1234 and len(ups) == 1                                             # uploaded once, as int32
    assert ups[0][1] == np.int32 and ups[0][0].dtype == np.int32 and ups[0][0].tolist() == [10, 50, 100, 99]
    for bad, msg in ((np.array([10, 50, 100]), 'one entry per signal'), (np.zeros((4, 1), int), 'one entry per signal'),
                     (np.array([10., 50., 100., 99.]), 'integers'), (np.array([9, 50, 100, 99]), 'need 0 <= start <= stop <= L'),
                     (np.array([10, 50, 101, 99]), 'need 0 <= start <= stop <= L')):
        with pytest.raises(ValueError, match=msg):
            eng._span_stops(bad, 4, 100, 10)
    with pytest.raises(ValueError, match='need 0 <= start'):
        eng._span_stops(np.array([10, 50, 100, 99]), 4, 100, -1)
    assert len(ups) == 1


def test_bss_estimates_argument_errors_come_before_any_launch():
    eng = _bare_engine([])
    y = np.zeros((2, 50), np.float32)
    with pytest.raises(ValueError, match='must all be .n_sig, L.'):
        eng.bss_estimates(y, y[:, :-1], y)
    with pytest.raises(ValueError, match='must all be .n_sig, L.'):
        eng.bss_estimates(y[0], y[0], y[0])
    with pytest.raises(ValueError, match='need 0 <= start <= L'):
        eng.bss_estimates(y, y, y, start=51)
    with pytest.raises(ValueError, match='need 0 <= start <= stop <= L'):
        eng.bss_estimates(y, y, y, start=10, stop=5)


def test_weighted_band_db_is_the_arithmetic_of_fw_snr_and_fw_sd():
    rng = np.random.default_rng(3)
    F, I = dm.band_importance(16000)
    num, den = 10.0 ** rng.uniform(-6, 1, (3, 2, len(F))), 10.0 ** rng.uniform(-6, 1, (3, 2, len(F)))
    for floor in (-15, 0):
        fq, mean = dm._weighted_band_db(num, den, I, floor)
        v = np.minimum(np.maximum(floor, 10 * np.log10(num) - 10 * np.log10(den)), 25)
        assert np.array_equal(fq, I / np.sum(I) * v) and np.array_equal(mean, np.sum(I / np.sum(I) * v, axis=-1))
        assert fq.shape == (3, 2, len(F)) and mean.shape == (3, 2)
    assert np.array_equal(dm._weighted_band_db(num, den, I, None)[0], I / np.sum(I) * (10 * np.log10(num) - 10 * np.log10(den)))
    # against the oracle's own statement of the same lines, given the oracle's levels
    x, n = rng.standard_normal(4000), 0.3 * rng.standard_normal(4000)
    b, a = meo.third_octave_filterbank(F, 16000, order=4)
    ls, ln = meo.band_levels(x, b, a), meo.band_levels(n, b, a)
    assert abs(dm._weighted_band_db(ls, ln, I, -15)[1] - meo.fw_snr(x, n, 16000)[1]) < 1e-12
    assert abs(dm._weighted_band_db(ln, ls, I, 0)[1] - meo.fw_sd(x, n, 16000)[1]) < 1e-12


def _batch(R=2, K=2, L=17000):
    return [np.zeros((R, K, L), np.float32) for _ in range(6)]


def test_batch_results_argument_errors():
    sig = _batch()
    snrs = np.zeros((2, 2))
    for lengths, msg in ((np.array([17000]), 'one integer per room'), (np.array([17000., 17000.]), 'one integer per room'),
                         (np.array([15999, 17000]), 'need fs = 16000 <= lengths <= 17000'), (np.array([16500, 17001]), 'need fs = 16000 <= lengths <= 17000')):
        with pytest.raises(ValueError, match=msg):
            rio.batch_results(*sig, snrs, lengths=lengths)
    with pytest.raises(ValueError, match='nf_t: expected leading axes .2, 2.'):
        rio.batch_results(*sig[:3], np.zeros((2, 3, 17000), np.float32), *sig[4:], snrs)
    with pytest.raises(ValueError, match='s_dry: expected leading axes .2,.'):
        rio.batch_results(*sig, snrs, s_dry=np.zeros((3, 17000), np.float32), n_dry=np.zeros((2, 17000), np.float32))
    import torch
    with pytest.raises(TypeError, match='every signal as a NumPy array or every signal as a device-resident torch tensor'):
        rio.batch_results(torch.zeros((2, 2, 17000)), *sig[1:], snrs)
    with pytest.raises(ValueError, match='sf_t: device tensors must be contiguous'):
        rio.batch_results(*(torch.zeros((2, 2, 17000)) for _ in range(2)), torch.zeros((2, 2, 34000))[..., ::2], *(torch.zeros((2, 2, 17000)) for _ in range(3)), snrs)


def test_results_of_room_takes_one_row_of_every_key():
    R, K = 3, 2
    res = {k: np.arange(R * K, dtype=float).reshape(R, K) + i for i, k in enumerate(rio.RESULT_KEYS_TANGO)}
    resz = {k: -(np.arange(R * K, dtype=float).reshape(R, K) + i) for i, k in enumerate(rio.RESULT_KEYS_MWF)}
    res['snr_in_raw'] = resz['snr_in_raw'] = [[1.0], [2.0], [3.0]]            # whatever the caller passed, indexed by room
    one, onez = rio.results_of_room(res, resz, 1)
    assert tuple(one) == rio.RESULT_KEYS_TANGO and tuple(onez) == rio.RESULT_KEYS_MWF
    for i, k in enumerate(rio.RESULT_KEYS_TANGO[1:], 1):
        assert np.array_equal(one[k], [2.0 + i, 3.0 + i])
    assert np.array_equal(one['snr_in_raw'], [2.0]) and np.array_equal(onez['delta_stoi'], -(np.array([2.0, 3.0]) + rio.RESULT_KEYS_MWF.index('delta_stoi')))
