"""The meeting-room kernels (csrc/k_roomsynth.h k_source_mix, csrc/k_stft.h k_source_masks) under the hipemu CPU emulator (no GPU): the checks
of tests/test_gpu_meeting.py through the same C ABI, Engine and package functions.  Cut down where the emulator is slow: the mask cases to
`mask_cases(cut=True)` (one per FFT size and padding, plus one that crosses a run edge), the SIRs to one room of three
single-microphone nodes, the dry sources of the rooms to 1100 samples.  Test tooling only; the real runs are -m gpu."""
import pytest

import emu_build
import meeting_checks as mk
from disco_amd import _engines, _lib
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk_(**cfg):
        return Engine(lib=lib, **cfg)
    return mk_


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


def test_emu_source_mix_bit_equality(make_engine):
    mk.check_source_mix_bits(make_engine)


def test_emu_source_mix_each_output_alone(make_engine):
    mk.check_source_mix_each_output_alone(make_engine)


def test_emu_source_mix_more_rows_than_the_grid(make_engine):
    mk.check_source_mix_many_rows(make_engine)


def test_emu_source_mix_nan_stays_in_its_channel(make_engine):
    mk.check_source_mix_nan_isolation(make_engine)


def test_emu_source_mix_refusals_write_nothing(make_engine):
    mk.check_source_mix_refusals(make_engine)


@pytest.mark.parametrize('case', mk.mask_cases(cut=True), ids=lambda c: f'{c[0]}-{c[1]}-S{c[2]}-T{c[3]}')
def test_emu_source_masks_against_the_float64_reference(make_engine, case):
    mk.check_mask_case(make_engine, case)


@pytest.mark.parametrize('n_fft,pad', [(512, 'reflect'), (1024, 'constant')])
def test_emu_source_masks_lengths(make_engine, n_fft, pad):
    mk.check_mask_lengths(make_engine, n_fft, pad)


def test_emu_source_masks_batch_independence(make_engine):
    mk.check_mask_batch_independence(make_engine, n_sig=4)


def test_emu_source_masks_refusals_write_nothing(make_engine):
    mk.check_mask_refusals(make_engine)


def test_emu_sir_at_nodes(emulated_package):
    mk.check_sir_at_nodes(cases=((3, (1, 1, 1)),), L=1200, R=1)


def test_emu_simulate_meetings(emulated_package):
    mk.check_simulate_meetings(Ld=1100, out_len=1700)


def test_emu_meeting_rooms_into_offline_tango(emulated_package):
    mk.check_meeting_rooms_tango(R=2, L=4096, lengths=(4096, 3000))


def test_emu_meeting_masks(make_engine, emulated_package):
    mk.check_meeting_masks(make_engine)
