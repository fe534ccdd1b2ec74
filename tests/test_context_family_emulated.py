"""The context family (a context and the two half-batch children of its overlapped whole-path calls) under the hipemu CPU emulator (no
GPU): tests/family_checks.py for every setter, applied before and after the children exist, and the device bytes the family owns after
every step of the sequence pinned to what the library gave before the host layer stated the family once (the emulator's "chip" has 3
compute units; the float64 step-1 chunk count of the wide shape follows that).  A characterisation: a change of the host code that
keeps this state cannot move it unnoticed.  Test tooling only; the real runs are -m gpu.
Wall time: about 2 minutes on an 8-core host (2 s per case of the small shape, 6 to 15 s per case of the wide one)."""
import pytest

import emu_build
import family_checks as fc
from disco_amd.engine import Engine

# (shape, setter, order) -> owned_bytes() after: creation, the first step, the second step, reserve(1)
OWNED = {
    ('fused-R3', 'tuning', 'before'): (2368512, 2368512, 3256704, 4343680),
    ('fused-R3', 'tuning', 'after'): (2368512, 4737024, 4737024, 5824000),
    ('fused-R3', 'packed_x', 'before'): (2368512, 2368512, 4737024, 5824000),
    ('fused-R3', 'packed_x', 'after'): (2368512, 4737024, 4737024, 5824000),
    ('fused-R3', 'lengths', 'before'): (2368512, 2368512, 4737024, 5824000),
    ('fused-R3', 'lengths', 'after'): (2368512, 4737024, 4737024, 5824000),
    ('fused-R3', 'stage_timing', 'before'): (2368512, 2368512, 4737024, 5824000),
    ('fused-R3', 'stage_timing', 'after'): (2368512, 4737024, 4737024, 5824000),
    ('fused-R2', 'tuning', 'before'): (1579008, 1579008, 2171136, 2896128),
    ('fused-R2', 'tuning', 'after'): (1579008, 3158016, 3158016, 3883008),
    ('fused-R2', 'packed_x', 'before'): (1579008, 1579008, 3158016, 3883008),
    ('fused-R2', 'packed_x', 'after'): (1579008, 3158016, 3158016, 3883008),
    ('fused-R2', 'lengths', 'before'): (1579008, 1579008, 3158016, 3883008),
    ('fused-R2', 'lengths', 'after'): (1579008, 3158016, 3158016, 3883008),
    ('fused-R2', 'stage_timing', 'before'): (1579008, 1579008, 3158016, 3883008),
    ('fused-R2', 'stage_timing', 'after'): (1579008, 3158016, 3158016, 3883008),
    ('wide-R3', 'tuning', 'before'): (17763840, 17763840, 31086720, 36269696),
    ('wide-R3', 'tuning', 'after'): (17763840, 35527680, 35527680, 40710656),
    ('wide-R3', 'room_cov', 'before'): (17763840, 17763840, 35527680, 40710656),
    ('wide-R3', 'room_cov', 'after'): (17763840, 35527680, 35527680, 40710656),
    ('wide-R3', 'fuse_wide_istft', 'before'): (17763840, 17763840, 35527680, 40710656),
    ('wide-R3', 'fuse_wide_istft', 'after'): (17763840, 35527680, 35527680, 40710656),
    ('wide-R3', 'lengths', 'before'): (17763840, 17763840, 35527680, 40710656),
    ('wide-R3', 'lengths', 'after'): (17763840, 35527680, 35527680, 40710656),
    ('wide-R3', 'stage_timing', 'before'): (17763840, 17763840, 35527680, 40710656),
    ('wide-R3', 'stage_timing', 'after'): (17763840, 35527680, 35527680, 40710656),
}


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()
    return lambda **cfg: Engine(lib=lib, **cfg)


def test_every_case_is_pinned():
    assert set(OWNED) == set(fc.cases())


@pytest.mark.parametrize('shape,setter,order', fc.cases(), ids=['-'.join(c) for c in fc.cases()])
def test_emu_children_follow(make_engine, shape, setter, order):
    owned = fc.check_setter(make_engine, shape, setter, order)
    print('family_owned', (shape, setter, order), owned)
    assert owned == OWNED[shape, setter, order]
