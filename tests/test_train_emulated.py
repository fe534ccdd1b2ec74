"""The training kernels under the hipemu CPU emulator (no GPU): gather, gate forward / backward, loss and its gradient, and the whole
model's gradients through the same autograd Functions with the emulated library bound (tests/train_checks.py)."""
import pytest

import emu_build
import train_checks as tc
from disco_amd import _lib


@pytest.fixture(scope='module')
def lib():
    return emu_build.load_emu()


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    assert _lib.takes_host_memory()
    yield


def test_emu_gather_fixture(lib):
    assert tc.check_gather_fixture(lib, 'cpu')


def test_emu_gather_257_and_refusals(lib):
    assert tc.check_gather_257_and_refusals(lib, 'cpu')


def test_emu_bank_gather(emulated_package):
    assert tc.check_bank_gather('cpu')


@pytest.mark.parametrize('later', [False, True])
@pytest.mark.parametrize('H', [3, 256])
def test_emu_gru_gates_train(lib, H, later):
    print('worst backward error / eps:', tc.check_gates(lib, 'cpu', 5, H, later))


def test_emu_gru_gates_off_the_16_byte_route(lib):
    print('worst backward error / eps:', tc.check_gates(lib, 'cpu', 5, 8, True, misalign=True))


def test_emu_gru_backward(lib):
    """What the two gate entry points refuse (the values are checked in test_emu_gru_gates_train)."""
    assert tc.check_gate_refusals(lib, 'cpu')


@pytest.mark.parametrize('part', ['all', 'mid', 'last'])
@pytest.mark.parametrize('F', [17, 257])
@pytest.mark.parametrize('C', [1, 4])
def test_emu_recon_loss(lib, C, F, part):
    print(tc.check_loss(lib, 'cpu', C, F, part, fixture=tc.golden() if F == 17 else None))


def test_emu_recon_loss_refusals(lib):
    assert tc.check_loss_refusals(lib, 'cpu')


@pytest.mark.parametrize('part', ['all', 'mid'])
@pytest.mark.parametrize('n_ch', [1, 4])
def test_emu_model_gradients(emulated_package, n_ch, part):
    print('new, plain:', tc.check_model_grads('cpu', n_ch, part))


def test_emu_kernel_route_is_taken(emulated_package, monkeypatch):
    assert tc.check_kernel_route_is_taken('cpu', monkeypatch)
