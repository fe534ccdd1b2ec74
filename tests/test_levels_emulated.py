"""The segmental-SNR and reverberation-ratio kernels (csrc/k_segsnr.h, csrc/k_reverb.h) under the hipemu CPU emulator (no GPU): the same
checks as tests/test_gpu_levels.py through the same C ABI, Engine, disco_amd.metrics, results_io and dataset_utils.rooms.  Test tooling
only; the real runs are -m gpu."""
import pytest

import emu_build
import reverb_checks as rc
import segsnr_checks as sg
from disco_amd import _engines, _lib


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


def test_emu_seg_snr_golden(emulated_package):
    sg.check_golden()


def test_emu_seg_snr_counts_clip_and_floor(emulated_package):
    sg.check_clip_and_floor_counts()


def test_emu_seg_snr_rows_alone_and_nan(emulated_package):
    sg.check_rows_alone_and_nan()


def test_emu_seg_snr_device_resident(emulated_package):
    sg.check_device_resident()


def test_emu_seg_snr_surface(emulated_package):
    sg.check_surface()


def test_emu_room_results_seg_snr_keys(emulated_package):
    sg.check_room_results()


def test_emu_batch_results_seg_snr_keys(emulated_package):
    sg.check_batch_results()


@pytest.mark.parametrize('k', range(len(rc.gen.REVERB_SHAPES)), ids=[f'{s[0]}x{s[1]}' for s in rc.gen.REVERB_SHAPES])
def test_emu_reverb_golden(emulated_package, k):
    rc.check_golden(k)


def test_emu_reverb_full_tail_against_rir_convolve(emulated_package):
    rc.check_full_tail_against_rir_convolve()


def test_emu_rir_split(emulated_package):
    rc.check_rir_split()


def test_emu_reverb_nan_containment(emulated_package):
    rc.check_nan_containment()


def test_emu_reverb_surface(emulated_package):
    rc.check_surface()


def test_emu_reverb_at_mics(emulated_package):
    rc.check_reverb_at_mics()
