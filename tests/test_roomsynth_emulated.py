"""The room-synthesis kernels (csrc/k_roomsynth.h) under the hipemu CPU emulator (no GPU): the checks of tests/test_gpu_roomsynth.py through
the same C ABI, Engine and package functions.  Cut down where the emulator is slow: the grid-stride mix at 66 000 rows of 4 samples, the
rooms at R = 2 and 4096 samples.  Test tooling only; the real runs are -m gpu."""
import pytest

import emu_build
import roomsynth_checks as rc
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


def test_emu_vad_against_the_reference(make_engine):
    rc.check_vad_golden(make_engine)


def test_emu_vad_window_count_edges(make_engine):
    rc.check_vad_window_edges(make_engine)


def test_emu_vad_window_settings(make_engine):
    rc.check_vad_settings(make_engine)


def test_emu_vad_stop_per_signal(make_engine):
    rc.check_vad_stops(make_engine)


def test_emu_vad_nan_stays_in_its_row(make_engine):
    rc.check_vad_nan_isolation(make_engine)


def test_emu_vad_and_ivad_mask_decide_alike(make_engine):
    rc.check_vad_against_ivad(make_engine)


def test_emu_vad_refusals_write_nothing(make_engine):
    rc.check_vad_refusals(make_engine)


def test_emu_mix_bit_equality(make_engine):
    rc.check_mix_bits(make_engine)


def test_emu_mix_unaligned_rows_and_in_place(make_engine):
    rc.check_mix_alignment_and_in_place(make_engine)


def test_emu_mix_more_rows_than_the_grid(make_engine):
    rc.check_mix_many_rows(make_engine, n_sig=66000, L=4)


def test_emu_mix_sum_is_not_fused(make_engine):
    rc.check_mix_no_fma(make_engine)


def test_emu_mix_refusals(make_engine):
    rc.check_mix_refusals(make_engine)


def test_emu_increase_to_snr_against_the_reference(emulated_package):
    rc.check_increase_to_snr()


def test_emu_increase_to_snr_fed_back(emulated_package):
    rc.check_increase_to_snr_feedback()


def test_emu_snr_at_mics_against_the_reference(emulated_package):
    rc.check_snr_at_mics()


def test_emu_simulate_rooms_and_valid_flags(emulated_package):
    rc.check_valid_flags(R=2, L=4096, base=rc.check_simulate_rooms(R=2, L=4096))


def test_emu_mix_rooms_into_offline_tango(emulated_package):
    rc.check_mix_rooms_tango(R=2, L=4096, lengths=(4096, 3000))


def test_emu_surface(emulated_package):
    rc.check_surface()
