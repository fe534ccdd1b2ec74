"""The packed workspace layout of X on the fused route of disco_tango_enhance (option "packed_x") on a real MI355X: equality of the two
layouts on every output, the float64 oracle on inputs that live in DC and Nyquist, per-room lengths, and the two covariance kernels
through their test-only entries (tests/packed_x_checks.py)."""
import pytest

import packed_x_checks as px
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('K,M', px.SHAPES)
def test_route_equal(make_engine, K, M):
    print(px.check_route_equal(make_engine, K, M, runs=((0, False), (0, True), (2, False), (2, True)), extras=True))


@pytest.mark.parametrize('K,M', [(4, 4), (3, 3)])
def test_dc_and_nyquist_are_there(make_engine, K, M):
    px.check_dc_nyquist(make_engine, K, M)


@pytest.mark.parametrize('overlap', [0, 2])
def test_per_room_lengths(make_engine, overlap):
    print(px.check_lengths(make_engine, overlap=overlap))


@pytest.mark.parametrize('K,M', [(4, 4), (3, 3), (2, 1), (2, 2), (5, 4), (2, 7)])
def test_kernels(make_engine, K, M):
    assert px.check_kernels(make_engine, K, M)


def test_no_allocation_in_a_compute_call(make_engine):
    assert px.check_no_allocation(make_engine)
