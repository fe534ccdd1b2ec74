"""The packed workspace layout of X (option "packed_x") under the hipemu CPU emulator (no GPU): the checks of tests/test_gpu_packed_x.py
through the same C ABI and Engine (tests/packed_x_checks.py), on the same shapes."""
import pytest

import emu_build
import packed_x_checks as px
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('K,M', px.SHAPES)
def test_emu_route_equal(make_engine, K, M):
    print(px.check_route_equal(make_engine, K, M, extras=(K, M) == (2, 2)))


@pytest.mark.parametrize('K,M', [(4, 4), (3, 3)])
def test_emu_dc_and_nyquist_are_there(make_engine, K, M):
    """room = 3: this is where the noise level of the inputs is confirmed -- the public layout passes with a factor 3 to spare"""
    px.check_dc_nyquist(make_engine, K, M, room=3.0)


def test_emu_per_room_lengths(make_engine):
    print(px.check_lengths(make_engine))


@pytest.mark.parametrize('K,M', [(4, 4), (3, 3), (2, 1), (2, 2)])
def test_emu_kernels(make_engine, K, M):
    assert px.check_kernels(make_engine, K, M)


def test_emu_no_allocation_in_a_compute_call(make_engine):
    assert px.check_no_allocation(make_engine)
