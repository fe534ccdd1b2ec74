"""The dry-source kernels (csrc/k_sources.h) under the hipemu CPU emulator (no GPU): the checks of tests/test_gpu_sources.py through the same
C ABI, Engine and package functions.  The transform is covered at EVERY n_fft = 2^10 ... 2^22 -- the emulator takes under a second per
signal even at 2^22 --, so every pass plan of src_plan() is run here, and the turned cosine at the smallest n_fft of each plan as on the
GPU.  Cut down where the emulator is slow: the grid-stride pass at 66 000 rows.  Test tooling only; the real runs are -m gpu."""
import pytest

import emu_build
import sources_checks as sc
from disco_amd import _engines, _lib
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


@pytest.mark.parametrize('p', sc.ALL_P)
def test_emu_noise_every_size(make_engine, p):
    sc.check_noise_sizes(make_engine, p)


@pytest.mark.parametrize('p', sc.PLAN_P)
def test_emu_noise_bin_placement(make_engine, p):
    sc.check_noise_placement(make_engine, p)


def test_emu_noise_dc_and_nyquist_keep_their_real_part(make_engine):
    sc.check_noise_dc_nyquist(make_engine)


def test_emu_noise_rows_do_not_see_each_other(make_engine):
    sc.check_noise_batch(make_engine)


def test_emu_noise_refusals_write_nothing(make_engine):
    sc.check_noise_refusals(make_engine)


def test_emu_affine_bit_equality(make_engine):
    sc.check_affine_bits(make_engine)


def test_emu_affine_stops_defaults_and_zeros(make_engine):
    sc.check_affine_stops(make_engine)


def test_emu_affine_more_rows_than_the_grid(make_engine):
    sc.check_affine_many_rows(make_engine, n_sig=66000)


def test_emu_affine_refusals_write_nothing(make_engine):
    sc.check_affine_refusals(make_engine)


def test_emu_noise_from_signal_against_the_reference(emulated_package):
    sc.check_noise_package()


def test_emu_target_segments_against_the_reference(emulated_package):
    sc.check_target_segments()


def test_emu_noise_segments(emulated_package):
    sc.check_noise_segments()


def test_emu_ssn_segments(emulated_package):
    sc.check_ssn_segments()


def test_emu_chain_from_dry_speech_to_tango(emulated_package):
    sc.check_chain()
