"""The training path on the CPU, no library bound: the restated helpers and the draws against the reference's records
(tests/golden/train_ref.npz), the bank, and forward_train / recon_loss_frames / fit through their torch fall-back
(tests/train_checks.py)."""
import pytest

import train_checks as tc


def test_helpers_match_the_reference_records():
    assert tc.check_helpers()


def test_draws_follow_the_reference_rules():
    assert tc.check_draws()


def test_bank_from_files(tmp_path):
    assert tc.check_from_files(tmp_path)


def test_bank_gather_cpu():
    assert tc.check_bank_gather('cpu')


@pytest.mark.parametrize('part', ['all', 'mid'])
@pytest.mark.parametrize('n_ch', [1, 4])
def test_model_gradients_cpu(n_ch, part):
    print('new, plain:', tc.check_model_grads('cpu', n_ch, part))


@pytest.mark.parametrize('n_ch', [1, 4])
def test_train_steps_cpu(n_ch):
    print('first, last loss:', tc.check_train_steps('cpu', n_ch))


def test_fit_cpu(tmp_path):
    print(tc.check_fit('cpu', tmp_path))
