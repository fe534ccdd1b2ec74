"""The training bank from rooms under the hipemu CPU emulator (no GPU): disco_bank_fill value by value through the C ABI, and
SpectraBank.from_rooms, dataset_utils.post and the round trip through the reference's files with the emulated library bound
(tests/bank_checks.py)."""
import pytest

import bank_checks as bc
import emu_build
from disco_amd import _engines, _lib


@pytest.fixture(scope='module')
def lib():
    return emu_build.load_emu()


@pytest.fixture(scope='module')
def emulated_package(lib):
    """The package's cached engines and wrappers on the emulated library for this module's tests; the references of bank_checks are shared
    among them."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, '_lib', lib)
        _engines._cache.clear()
        assert _lib.takes_host_memory()
        yield
        _engines._cache.clear()


def test_emu_fill_main_case(lib):
    print('worst error / 2^-22:', bc.check_main_case(lib, 'cpu') / bc.REL)


@pytest.mark.parametrize('name', sorted(bc.VARIANTS))
def test_emu_fill_variants(lib, name):
    print('worst error / 2^-22:', bc.check_variant(lib, 'cpu', name) / bc.REL)


def test_emu_fill_refusals(lib):
    assert bc.check_refusals(lib, 'cpu')


@pytest.mark.parametrize('z_sigs', ['zs_hat', None, ['zs_hat', 'zn_hat']], ids=['zs_hat', 'none', 'both'])
def test_emu_from_rooms_against_the_paths_outputs(emulated_package, z_sigs):
    print('worst error / 2^-22:', bc.check_from_rooms(z_sigs))


def test_emu_rooms_per_call(emulated_package):
    assert bc.check_rooms_per_call()


def test_emu_device_resident_inputs(emulated_package):
    assert bc.check_device_inputs('cpu')


def test_emu_bad_inputs(emulated_package):
    assert bc.check_bad_inputs()


def test_emu_batches_and_a_training_step(emulated_package):
    print('loss:', bc.check_batches_and_a_training_step())


def test_emu_round_trip_through_the_files(emulated_package, tmp_path):
    print('worst error / 2^-22:', bc.check_round_trip(tmp_path))


def test_emu_post_process_at_another_channel(emulated_package):
    assert bc.check_post_channel()
