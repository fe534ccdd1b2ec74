"""The STOI kernels (csrc/k_stoi.h) under the hipemu CPU emulator (no GPU): the same checks as tests/test_gpu_stoi.py through the same
C ABI, Engine and disco_amd.metrics, at spans of 1 - 1.5 s.  Test tooling only; the real runs are -m gpu.  The span the reference
scores (9 s) and the room through the whole path are left to the GPU file."""
import pytest

import emu_build
import stoi_checks as sc
from disco_amd import _engines, _lib


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


@pytest.mark.parametrize('fs,n', sc.CASES)
def test_emu_against_yardstick(emulated_package, fs, n):
    sc.check_against_yardstick(fs, n)


def test_emu_frame_count_edges(emulated_package):
    sc.check_frame_count_edges()


def test_emu_all_zero_x(emulated_package):
    sc.check_all_zero_x()


def test_emu_bit_identity(emulated_package):
    sc.check_bit_identity(n=9603)


def test_emu_device_resident(emulated_package):
    sc.check_device_resident()


def test_emu_room_results_stoi_keys(emulated_package, tmp_path):
    sc.check_room_results(tmp_path)
