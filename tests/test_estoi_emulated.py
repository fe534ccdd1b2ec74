"""The ESTOI kernels (csrc/k_estoi.h) under the hipemu CPU emulator (no GPU): the same checks as tests/test_gpu_estoi.py through the same
C ABI, Engine and disco_amd.metrics, at spans of 1 - 1.5 s.  Test tooling only; the real runs are -m gpu.  The span the reference
scores (9 s) is left to the GPU file."""
import pytest

import emu_build
import estoi_checks as ec
from disco_amd import _engines, _lib


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


@pytest.mark.parametrize('fs,n', ec.CASES)
def test_emu_against_yardstick(emulated_package, fs, n):
    ec.check_against_yardstick(fs, n)


def test_emu_bands_frame_counts(emulated_package):
    ec.check_bands_frame_counts()


def test_emu_bands_degenerate(emulated_package):
    ec.check_bands_degenerate()


def test_emu_frame_count_edges(emulated_package):
    ec.check_frame_count_edges()


def test_emu_all_zero_x_and_identity(emulated_package):
    ec.check_all_zero_x_and_identity()


def test_emu_bit_identity(emulated_package):
    ec.check_bit_identity(n=9603)


def test_emu_device_resident(emulated_package):
    ec.check_device_resident()


def test_emu_room_results_estoi_keys(emulated_package, tmp_path):
    ec.check_room_results(tmp_path)


def test_emu_batch_results_estoi_keys(emulated_package):
    ec.check_batch_results()


def test_emu_surface(emulated_package):
    ec.check_surface()
