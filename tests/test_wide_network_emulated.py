"""The wide-network route (step-2 pencils of 17 <= P <= 32 channels: csrc/k_cov_wide.h, csrc/k_solve_wide.h, k_apply_m<M, 31>) under
the hipemu CPU emulator (no GPU), at reduced sizes: the checks of tests/test_gpu_wide_network.py through the same C ABI and Engine."""
import pytest

import emu_build
import wide_checks as wc
from disco_amd.engine import DiscoError, Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_wide_solver_full_matrices(make_engine):
    print(wc.check_solver_full(make_engine, sizes=(17, 19, 24, 31, 32), n=5))


def test_emu_wide_solver_indefinite(make_engine):
    import parity_checks as pc
    print(pc.check_solver_indefinite(make_engine, sizes=(17, 32), per_case=2, cross=1))


def test_emu_wide_solver_small_gap(make_engine):
    print(wc.check_solver_small_gap(make_engine, sizes=(17, 32), gaps=(0.9,), n=2))


def test_emu_wide_solver_nan_neighbours(make_engine):
    assert wc.check_solver_nan_neighbours(make_engine, P=18, n=9)


@pytest.mark.parametrize('K,M', [(16, 2), (6, 4), (17, 1)])
def test_emu_wide_solver_from_partials(make_engine, K, M):
    print(wc.check_solver_from_partials(make_engine, K, M))


@pytest.mark.parametrize('K,M', [(16, 2), (10, 8)])
def test_emu_wide_staged(make_engine, K, M):
    print(wc.check_staged(make_engine, K, M))


def test_emu_wide_end_to_end(make_engine):
    print(wc.check_end_to_end(make_engine, R=1, K=16, M=2, L=(4 * 17 + 3) * 256))


def test_emu_wide_refusals(make_engine):
    assert wc.check_refusals(make_engine, DiscoError)
