"""Rooms of different clip lengths in one batch (disco_set_lengths) under the hipemu CPU emulator (no GPU), at reduced sizes: the checks
of tests/test_gpu_mixed_lengths.py through the same C ABI and Engine (tests/length_checks.py)."""
import pytest

import emu_build
import length_checks as lc
from disco_amd import _engines, _lib
from disco_amd.engine import DiscoError, Engine


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


@pytest.mark.parametrize('n_fft,pad_mode,chans', [(512, 'reflect', 1), (512, 'constant', 2), (512, 'reflect', 4), (512, 'reflect', 5),
                                                  (512, 'constant', 8), (1024, 'reflect', 1), (1024, 'constant', 2), (1024, 'reflect', 4),
                                                  (1024, 'reflect', 5), (1024, 'reflect', 8)])
def test_emu_stft_at_the_edges(make_engine, n_fft, pad_mode, chans):
    print(lc.check_stft_edges(make_engine, n_fft, pad_mode, chans))


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_emu_istft_at_the_edges(make_engine, n_fft):
    print(lc.check_istft_edges(make_engine, n_fft))


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_emu_mask_oracle_at_the_edges(make_engine, n_fft):
    print(lc.check_mask_edges(make_engine, n_fft, masks=('irm1', 'iam1', 'ibm1')))


def test_emu_cov_mean_over_own_frames(make_engine):
    assert lc.check_cov_mean(make_engine)


def test_emu_whole_path_single_node(make_engine):
    lc.check_whole_path(make_engine, 1, 4, lc.LENGTHS_K3M2[:3], want_stage='stft_apply_istft')


@pytest.mark.parametrize('staged', [False, True])
def test_emu_whole_path_k3m2(make_engine, staged):
    lc.check_whole_path(make_engine, 3, 2, lc.LENGTHS_K3M2, staged_step2=staged, tuning=(8, 2, 2, 4),
                        want_stage='cov2' if staged else 'step2_apply_istft')


def test_emu_whole_path_k3m2_overlapped(make_engine):
    lc.check_whole_path(make_engine, 3, 2, lc.LENGTHS_K3M2, overlap=2, alone=False)


def test_emu_whole_path_k4m4(make_engine):
    lc.check_whole_path(make_engine, 4, 4, (12288, 8193, 10000), alone=False)


def test_emu_whole_path_room_pass(make_engine):
    lc.check_whole_path(make_engine, 2, 8, (12288, 10000, 11100), want_stage='room_cov2', alone=False)


def test_emu_whole_path_room_pass_iterated(make_engine):
    lc.check_whole_path(make_engine, 2, 8, (21504, 20100, 22023), n_fft=1024, iters=2, want_stage='apply2_istft', alone=False)


def test_emu_whole_path_wide(make_engine):
    lc.check_whole_path(make_engine, 16, 2, ((4 * 17 + 4) * 256, (4 * 17 + 3) * 256 + 100), alone=False)


def test_emu_alone_equals_batched_near_a_whole_hop(make_engine):
    lc.check_alone_equals_batched_near_whole_hop(make_engine)


def test_emu_tango_reference_every_mode(make_engine):
    lc.check_reference_outputs(make_engine, lengths=lc.LENGTHS_K3M2[:4])


def test_emu_uniform_batch_untouched(make_engine):
    assert lc.check_uniform_untouched(make_engine, L=6000, R=2)


def test_emu_refusals_and_arguments(make_engine):
    assert lc.check_refusals(make_engine, DiscoError)


def test_emu_python_surface(emulated_package):
    lc.check_python_surface()
