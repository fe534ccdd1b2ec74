"""Dry sources prepared on a real MI355X (tests/sources_checks.py): the long real transform with random phases (disco_noise_from_signal)
at every n_fft = 2^10 ... 2^22 against its float64 statement under a bar set by a float32 CPU transform, a turned cosine on the bins
around every pass boundary, the DC and Nyquist bins, the batch structure and the refusals; the subtract-scale-shift-wrap pass
(disco_affine_segment) bit for bit on both access routes; next to them noise_from_signal, target_segments, noise_segments and ssn_segments
against the reference's own outputs, and one chain from dry speech to offline_tango_batched that never leaves the device.
Kernels launched here: k_src_wave_pass<512 | 1024, 1 | 4>, k_src_small_pass<4 | 8 | 16>, k_src_mid, k_src_zero_tail,
k_affine_segment<true | false>, and those of the room-synthesis and reference paths."""
import pytest

import sources_checks as sc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('p', sc.ALL_P)
def test_noise_every_size(make_engine, p):
    sc.check_noise_sizes(make_engine, p)


@pytest.mark.parametrize('p', sc.PLAN_P)
def test_noise_bin_placement(make_engine, p):
    sc.check_noise_placement(make_engine, p)


def test_noise_dc_and_nyquist_keep_their_real_part(make_engine):
    sc.check_noise_dc_nyquist(make_engine)


def test_noise_rows_do_not_see_each_other(make_engine):
    sc.check_noise_batch(make_engine)


def test_noise_refusals_write_nothing(make_engine):
    sc.check_noise_refusals(make_engine)


def test_affine_bit_equality(make_engine):
    sc.check_affine_bits(make_engine)


def test_affine_stops_defaults_and_zeros(make_engine):
    sc.check_affine_stops(make_engine)


def test_affine_more_rows_than_the_grid(make_engine):
    sc.check_affine_many_rows(make_engine)


def test_affine_refusals_write_nothing(make_engine):
    sc.check_affine_refusals(make_engine)


def test_noise_from_signal_against_the_reference():
    sc.check_noise_package()


def test_target_segments_against_the_reference():
    sc.check_target_segments()


def test_noise_segments():
    sc.check_noise_segments()


def test_ssn_segments():
    sc.check_ssn_segments()


def test_chain_from_dry_speech_to_tango():
    sc.check_chain()
