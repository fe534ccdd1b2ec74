"""The training bank from rooms on the MI355X: disco_bank_fill (k_bank_fill) value by value through the C ABI, SpectraBank.from_rooms against
the path's own outputs, in pieces, from device-resident rooms, into batches and one training step, and the round trip through the
reference's files (tests/bank_checks.py)."""
import pytest

import bank_checks as bc
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    import torch
    torch.cuda.set_device(0)
    return 'cuda:0'


def test_fill_main_case(dev):
    print('worst error / 2^-22:', bc.check_main_case(_lib.load(), dev) / bc.REL)


@pytest.mark.parametrize('name', sorted(bc.VARIANTS))
def test_fill_variants(dev, name):
    print('worst error / 2^-22:', bc.check_variant(_lib.load(), dev, name) / bc.REL)


def test_fill_refusals(dev):
    assert bc.check_refusals(_lib.load(), dev)


@pytest.mark.parametrize('z_sigs', ['zs_hat', None, ['zs_hat', 'zn_hat']], ids=['zs_hat', 'none', 'both'])
def test_from_rooms_against_the_paths_outputs(dev, z_sigs):
    print('worst error / 2^-22:', bc.check_from_rooms(z_sigs))


def test_rooms_per_call(dev):
    assert bc.check_rooms_per_call()


def test_device_resident_inputs(dev):
    assert bc.check_device_inputs(dev)


def test_bad_inputs(dev):
    assert bc.check_bad_inputs()


def test_batches_and_a_training_step(dev):
    print('loss:', bc.check_batches_and_a_training_step())


def test_round_trip_through_the_files(dev, tmp_path):
    print('worst error / 2^-22:', bc.check_round_trip(tmp_path))


def test_post_process_at_another_channel(dev):
    assert bc.check_post_channel()
