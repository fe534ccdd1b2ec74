"""Segmental SNR (disco_seg_snr, csrc/k_segsnr.h) and the reverberation ratios (disco_rir_split, disco_reverb_energies, csrc/k_reverb.h) on a
real MI355X against the reference's own values (tests/golden/levels_ref.npz): every window size and span length of the list, the VAD
weights, spans and NaN containment bit for bit, the keys of room_results / batch_results; every (dry length, response length) and split
position of the list, rows alone and in the batch bit for bit, the energy against Engine.rir_convolve, the split rules, the refusals.
Kernels launched here: k_seg_snr, k_rir_split, k_reverb_spectra, k_reverb_mac_energy<8 | 16>, k_conv_*, k_vad_samples, k_band_stats."""
import pytest

import reverb_checks as rc
import segsnr_checks as sg
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gfx950_library():
    _lib.load()          # raises if the gfx950 library is missing: no fallback


def test_seg_snr_golden():
    sg.check_golden()


def test_seg_snr_counts_clip_and_floor():
    sg.check_clip_and_floor_counts()


def test_seg_snr_rows_alone_and_nan():
    sg.check_rows_alone_and_nan()


def test_seg_snr_device_resident():
    sg.check_device_resident()


def test_seg_snr_surface():
    sg.check_surface()


def test_room_results_seg_snr_keys():
    sg.check_room_results()


def test_batch_results_seg_snr_keys():
    sg.check_batch_results()


@pytest.mark.parametrize('k', range(len(rc.gen.REVERB_SHAPES)), ids=[f'{s[0]}x{s[1]}' for s in rc.gen.REVERB_SHAPES])
def test_reverb_golden(k):
    rc.check_golden(k)


def test_reverb_full_tail_against_rir_convolve():
    rc.check_full_tail_against_rir_convolve()


def test_rir_split():
    rc.check_rir_split()


def test_reverb_nan_containment():
    rc.check_nan_containment()


def test_reverb_surface():
    rc.check_surface()


def test_reverb_at_mics():
    rc.check_reverb_at_mics()
