"""Meeting rooms of several talkers on a real MI355X (tests/meeting_checks.py): the leave-one-out mixes (disco_source_mix) bit for bit
against NumPy float32 sums in the stated order, on both access routes, at every stop, with NaN beyond the stops and inside one channel;
the per-source masks and the mix spectrum (disco_source_masks) bin by bin against the float64 reference in the reference's own order of
operations, for both FFT sizes and paddings, one pair to four pairs of sources, a lone last source, every run edge; per-room lengths and
batch independence bit for bit; sir_at_nodes, simulate_meetings, meeting_rooms into offline_tango_batched, meeting_masks.
Kernels launched here: k_source_mix<true | false>, k_source_masks<512 | 1024, 1..4, prefetch | none>, k_mix_scaled, k_ism_rir, k_conv_*,
the BSS-eval kernels, k_mask_oracle's reference path and the whole reference path."""
import pytest

import meeting_checks as mk
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk_(**cfg):
        return Engine(lib=lib, **cfg)
    return mk_


def test_source_mix_bit_equality(make_engine):
    mk.check_source_mix_bits(make_engine)


def test_source_mix_each_output_alone(make_engine):
    mk.check_source_mix_each_output_alone(make_engine)


def test_source_mix_more_rows_than_the_grid(make_engine):
    mk.check_source_mix_many_rows(make_engine)


def test_source_mix_nan_stays_in_its_channel(make_engine):
    mk.check_source_mix_nan_isolation(make_engine)


def test_source_mix_refusals_write_nothing(make_engine):
    mk.check_source_mix_refusals(make_engine)


@pytest.mark.parametrize('case', mk.mask_cases(), ids=lambda c: f'{c[0]}-{c[1]}-S{c[2]}-T{c[3]}')
def test_source_masks_against_the_float64_reference(make_engine, case):
    mk.check_mask_case(make_engine, case)


@pytest.mark.parametrize('n_fft,pad', [(512, 'reflect'), (512, 'constant'), (1024, 'reflect'), (1024, 'constant')])
def test_source_masks_lengths(make_engine, n_fft, pad):
    mk.check_mask_lengths(make_engine, n_fft, pad)
    mk.check_mask_lengths(make_engine, n_fft, pad, S=8, kind='iam1')


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_source_masks_batch_independence(make_engine, n_fft):
    mk.check_mask_batch_independence(make_engine, n_fft)


def test_source_masks_refusals_write_nothing(make_engine):
    mk.check_mask_refusals(make_engine)


def test_sir_at_nodes():
    mk.check_sir_at_nodes()


def test_sir_valid_and_value_range():
    mk.check_sir_valid_golden()


def test_simulate_meetings():
    mk.check_simulate_meetings()


def test_meeting_rooms_into_offline_tango():
    mk.check_meeting_rooms_tango()


def test_meeting_masks(make_engine):
    mk.check_meeting_masks(make_engine)
