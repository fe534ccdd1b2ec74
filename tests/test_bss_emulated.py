"""The BSS-eval kernels (csrc/k_bss.h) under the hipemu CPU emulator (no GPU), at small sizes: the same checks as
tests/test_gpu_bss.py through the same C ABI, Engine and disco_amd.metrics.  Test tooling only; the real runs are -m gpu.
Filter lengths here are 1, 8 and 64 with up to three sources (N = nsrc flen <= 192, the blocked factorisation crosses six tiles), plus
ONE case at mir_eval's 512 taps (N = 1024, some 15 s under the emulator); the other full-size cases and full-length signals are left
to the GPU file."""
import pytest

import bss_checks as bc
import emu_build
from disco_amd import _engines, _lib


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


@pytest.mark.parametrize('nsrc', (1, 2, 3))
@pytest.mark.parametrize('flen', (1, 8, 64))
def test_emu_spectra_against_dense(emulated_package, flen, nsrc):
    bc.check_against_oracle(bc.SPECTRA, 3000, flen, nsrc, cond_max=1e7)


@pytest.mark.parametrize('nsrc', (1, 2, 3))
@pytest.mark.parametrize('flen', (1, 8, 64))
def test_emu_noise_floor_1e5_against_dense(emulated_package, flen, nsrc):
    bc.check_against_oracle(('floor1e-5',), 5000, flen, nsrc, cond_max=1e11)


def test_emu_noise_floor_1e5_flen512_against_dense(emulated_package):
    bc.check_against_oracle(('floor1e-5',), 6000, 512, 2, cond_max=1e11)


def test_emu_closed_forms(emulated_package):
    bc.check_closed_forms(6000, 128)


def test_emu_permutation(emulated_package):
    bc.check_permutation(3000, 16)


def test_emu_batching_bit_identical(emulated_package):
    bc.check_batching(1500, 8)


def test_emu_more_than_one_time_chunk(emulated_package):
    """40 000 samples: three time chunks per pair, the last one partial."""
    bc.check_against_oracle(('fir',), 40000, 8, 2, oracle='gram', cond_max=1e7)


def test_emu_start_stop_and_mixed_lengths(emulated_package):
    bc.check_start_stop_and_lengths(4000, 24)


def test_emu_refusals(emulated_package):
    bc.check_refusals(2000)


def test_emu_lag_corr(emulated_package):
    bc.check_lag_corr(2500)


def test_emu_room_results_bss_keys(emulated_package, tmp_path):
    bc.check_room_results(64, tmp_path)
