"""From reverberated sources to rooms on a real MI355X (tests/roomsynth_checks.py): the per-sample VAD (disco_vad_samples) sample by sample
against the reference and the NumPy statement of its arithmetic, at every window-count edge, window setting and stop; the scaled mix
(disco_mix_scaled) bit for bit on both access routes and without a fused multiply-add; increase_to_snr and snr_at_mics against the
reference's own outputs; simulate_rooms against the same public calls made by hand; mix_rooms into offline_tango_batched.
Kernels launched here: k_vad_samples, k_mix_scaled<true | false>, k_vad_mask, k_band_stats, k_ism_rir, k_conv_*, and the reference path."""
import pytest

import roomsynth_checks as rc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_vad_against_the_reference(make_engine):
    rc.check_vad_golden(make_engine)


def test_vad_window_count_edges(make_engine):
    rc.check_vad_window_edges(make_engine)


def test_vad_window_settings(make_engine):
    rc.check_vad_settings(make_engine)


def test_vad_stop_per_signal(make_engine):
    rc.check_vad_stops(make_engine)


def test_vad_nan_stays_in_its_row(make_engine):
    rc.check_vad_nan_isolation(make_engine)


def test_vad_and_ivad_mask_decide_alike(make_engine):
    rc.check_vad_against_ivad(make_engine)


def test_vad_refusals_write_nothing(make_engine):
    rc.check_vad_refusals(make_engine)


def test_mix_bit_equality(make_engine):
    rc.check_mix_bits(make_engine)


def test_mix_unaligned_rows_and_in_place(make_engine):
    rc.check_mix_alignment_and_in_place(make_engine)


def test_mix_more_rows_than_the_grid(make_engine):
    rc.check_mix_many_rows(make_engine)


def test_mix_sum_is_not_fused(make_engine):
    rc.check_mix_no_fma(make_engine)


def test_mix_refusals(make_engine):
    rc.check_mix_refusals(make_engine)


def test_increase_to_snr_against_the_reference():
    rc.check_increase_to_snr()


def test_increase_to_snr_fed_back():
    rc.check_increase_to_snr_feedback()


def test_snr_at_mics_against_the_reference():
    rc.check_snr_at_mics()


def test_simulate_rooms_and_valid_flags():
    rc.check_valid_flags(base=rc.check_simulate_rooms())


def test_mix_rooms_into_offline_tango():
    rc.check_mix_rooms_tango()


def test_surface():
    rc.check_surface()
