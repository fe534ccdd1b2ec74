"""The context family (a context and the two half-batch children of its overlapped whole-path calls) on a real MI355X
(tests/family_checks.py): under every setter -- the tuning, each option that changes the route at the shape, per-room lengths and their
removal, the stage timers --, applied before and after the children exist, the overlapped call equals the plain call bit for bit, every
stage is launched twice over all rooms, and no whole-path call after reserve(1) allocates."""
import pytest

import family_checks as fc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback
    return lambda **cfg: Engine(lib=lib, **cfg)


@pytest.mark.parametrize('shape,setter,order', fc.cases(), ids=['-'.join(c) for c in fc.cases()])
def test_children_follow(make_engine, shape, setter, order):
    owned = fc.check_setter(make_engine, shape, setter, order)
    assert owned[-1] >= owned[-2] >= owned[0]
