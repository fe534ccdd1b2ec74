"""The kernels that feed the path and score it on a real MI355X, value by value (tests/mask_metric_checks.py): the TF masks on every
accepted name, across the float32 range, on the special inputs and the planted 'ibm' ties, at every launch-geometry edge; the
per-channel masks of the whole path bit for bit; the oracle masks from time signals bin by bin at every run boundary; the VAD mask
frame by frame on six signal families at every length edge up to the 4096 hops the kernel holds; the level statistics count by count
and sum by sum at every signals-per-workgroup edge, and through disco_amd.metrics.

Kernels launched here: k_tf_mask, k_tf_mask_channel (through disco_tango_reference, with the path's own kernels around it),
k_mask_oracle<512>, k_mask_oracle<1024>, k_stft<512>, k_vad_mask, k_pair_stats, k_band_stats<false>, k_band_stats<true>.
Lines starting with "mask_metrics" carry what the GPU showed (profiles/mask_metrics_errors.json).
31 tests, 6 s on an MI355X (most of it the float64 and long-double references on the host)."""
import json

import pytest

import mask_metric_checks as mc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def _report(family, value):
    print('mask_metrics_errors', json.dumps({family: value}))


def test_every_accepted_mask_name(make_engine):
    """irm, iam, ibm x 0..9 on 3000 Gaussian elements, 'ibm' at -6, 0 and 3 dB: worst err / bar per type."""
    _report('elementwise_worst_err_over_bar', mc.check_every_name(make_engine))


def test_magnitude_sweep(make_engine):
    """|S| from 1e-38 to 1e38: the bar where the inputs are finite, NaN and inf exactly where the float32 reference has them."""
    _report('magnitude_sweep_worst_err_over_bar', mc.check_magnitude_sweep(make_engine))


def test_special_inputs(make_engine):
    mc.check_special_inputs(make_engine)


def test_ibm_ties(make_engine):
    """N = S, -S, conj(S), i S at 0 dB: the reference answers 1 on every one."""
    _report('ibm_ties_fraction_answered_1', mc.check_ibm_ties(make_engine))


def test_launch_geometry(make_engine):
    """n = 1, 255, 256, 257, and beyond the 16384 x 256 elements of one grid (the stride loop)."""
    _report('geometry_worst_err_over_bar', mc.check_geometry(make_engine))


def test_mask_of_a_concatenation(make_engine):
    mc.check_mask_batch_independence(make_engine)


@pytest.mark.parametrize('M', (1, 2, 3, 8))
def test_per_channel_masks_of_the_path(make_engine, M):
    """masks_z at ref_mic in {0, M - 1} and mask_w at channel 0, bit for bit Engine.tf_mask of that channel's spectra."""
    for m, ref_mic, kind in mc.channel_cases((M,)):
        mc.check_channel_masks(make_engine, m, ref_mic, kind)


def test_masks_z_with_compressed_rows(make_engine):
    """mask_for_z = 'compressed' leaves masks_z the step-1 mask (its own k_tf_mask output stays in the workspace)."""
    mc.check_compressed_masks(make_engine)


@pytest.mark.parametrize('pad', ('reflect', 'constant'))
@pytest.mark.parametrize('n_fft', (512, 1024))
def test_oracle_masks_from_time_signals(make_engine, n_fft, pad):
    """Every bin of every frame, 15 .. 65 frames, 1, 3 and 5 signals: the kernel's worst err / (delta G) beside the float32 restatement's."""
    cases = [c for c in mc.oracle_cases() if c[:2] == (n_fft, pad)]
    assert len(cases) == 6
    worst = max(mc.check_oracle_case(make_engine, c) for c in cases)
    _report(f'oracle_masks_k_mask_oracle<{n_fft}>_{pad}', {'kernel_worst_ratio': round(worst, 4), 'f32_restatement_worst_ratio': round(mc.f32_restatement_ratio(cases), 4),
                                                          'C': mc.C_ORACLE})


@pytest.mark.parametrize('n_fft', (512, 1024))
def test_vad_mask(make_engine, n_fft):
    frames = sum(mc.check_vad(make_engine, n_fft, L) for L in mc.vad_lengths(n_fft))
    _report(f'vad_{n_fft}', {'frames_compared': frames, 'frames_wrong': 0})


def test_vad_mask_at_4096_hops(make_engine):
    """1 048 576 samples: the most the LDS counters hold."""
    mc.check_vad(make_engine, 512, 4096 * 256, alone=(3,))


def test_vad_refusal_leaves_the_context_usable(make_engine):
    mc.check_vad_refusal(make_engine)


def test_pair_stats(make_engine):
    _report('pair_stats_worst_abs_err', mc.check_pair_stats(make_engine))


@pytest.mark.parametrize('bank', mc.BANKS)
def test_band_stats(make_engine, bank):
    """Six spans x n_sig in {1, spb, spb + 1, 2 spb + 1} x ungated and gated."""
    res = {str(span): mc.check_band_case(make_engine, bank, span) for span in mc.SPANS}
    _report(f'band_stats_{bank}', res[str(mc.SPANS[0])])


def test_band_rows_alone(make_engine):
    mc.check_band_rows_alone(make_engine)
    mc.check_band_rows_alone(make_engine, bank=100, span=(257, 0, 257))
    mc.check_band_rows_alone(make_engine, bank=7, span=(700, 0, 700))


def test_metrics_batch():
    _report('metrics_batch_worst_dB', mc.check_metrics_batch())
