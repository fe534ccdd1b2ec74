"""The training path on the MI355X: the five kernels value by value, the whole model's gradients through them against float64 and
against the nn.GRU route, training steps and fit (tests/train_checks.py)."""
import pytest

import train_checks as tc
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    import torch
    torch.cuda.set_device(0)
    return 'cuda:0'


def test_gather_fixture(dev):
    assert tc.check_gather_fixture(_lib.load(), dev)


def test_gather_257_and_refusals(dev):
    assert tc.check_gather_257_and_refusals(_lib.load(), dev)


def test_bank_gather(dev):
    assert tc.check_bank_gather(dev)


@pytest.mark.parametrize('later', [False, True])
@pytest.mark.parametrize('H', [3, 256])
def test_gru_gates_train_and_backward(dev, H, later):
    print('worst backward error / eps:', tc.check_gates(_lib.load(), dev, 5, H, later))


def test_gru_gates_off_the_16_byte_route(dev):
    print('worst backward error / eps:', tc.check_gates(_lib.load(), dev, 5, 8, True, misalign=True))


def test_gate_refusals(dev):
    assert tc.check_gate_refusals(_lib.load(), dev)


@pytest.mark.parametrize('part', ['all', 'mid', 'last'])
@pytest.mark.parametrize('F', [17, 257])
@pytest.mark.parametrize('C', [1, 4])
def test_recon_loss(dev, C, F, part):
    print(tc.check_loss(_lib.load(), dev, C, F, part, fixture=tc.golden() if F == 17 else None))


def test_recon_loss_refusals(dev):
    assert tc.check_loss_refusals(_lib.load(), dev)


@pytest.mark.parametrize('part', ['all', 'mid'])
@pytest.mark.parametrize('n_ch', [1, 4])
def test_model_gradients(dev, n_ch, part):
    print('new, plain:', tc.check_model_grads(dev, n_ch, part))


@pytest.mark.parametrize('n_ch,part', [(1, 'all'), (4, 'mid')])
def test_model_gradients_native_convolutions(dev, n_ch, part):
    """The same check with torch's own convolution / BatchNorm kernels: both routes within 2e-6 of float64 there (the library's kernels put
    both 4 to 12 % away at this batch, see train_checks.py), so that the 3 x bar has teeth on the GPU too."""
    print('new, plain:', tc.check_model_grads(dev, n_ch, part, native_conv=True))


def test_kernel_route_is_taken(dev, monkeypatch):
    assert tc.check_kernel_route_is_taken(dev, monkeypatch)


@pytest.mark.parametrize('n_ch', [1, 4])
def test_train_steps(dev, n_ch):
    print('first, last loss:', tc.check_train_steps(dev, n_ch))


def test_fit(dev, tmp_path):
    print(tc.check_fit(dev, tmp_path))
