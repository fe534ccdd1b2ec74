"""The room pass, the split kernels that skip the step-1 block and the re-use route of the fused step 2 under the hipemu CPU emulator (no
GPU): the exact tier of tests/test_gpu_room_routes.py through the same C ABI and Engine, cut to (8, 2) and (4, 6) at 512 points with
three frame counts, one 1024-point room, one mixed-length batch, store_z = 0, one split shape per M, two re-use shapes, NaN beyond the
own frames of the rooms of a mixed-length batch and the containment of a NaN.  Test tooling only; the real runs are -m gpu.
Wall time: about 40 s on an 8-core host."""
import pytest

import emu_build
import room_checks as rc
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()
    return lambda **cfg: Engine(lib=lib, **cfg)


CASES = rc.staged_cases(cut=True)


def test_emu_cut_covers_both_routes_and_every_split_table():
    names = rc.launched_by(CASES)
    assert {'k_room_cov_dma<8,2,8>', 'k_room_cov_dma<4,6,8>'} <= names
    for M in (8, 4, 2):
        assert any(n.startswith(f'k_cov_split_lds<{M},') and n.endswith(',true>') for n in names), M
    assert any(c['n_fft'] == 1024 for c in CASES) and any(c.get('frames') and 1 in c['frames'] for c in CASES)
    assert any(c.get('store_z') is False for c in CASES) and len({c['T'] for c in CASES if c['room_cov']}) >= 3
    assert any(min(c.get('frames') or (c['T'],)) >= 4 * (c['M'] + c['K'] - 1) for c in CASES if c['room_cov'])       # a pending solve ...
    assert any(c['T'] >= 4 * (c['M'] + c['K'] - 1) for c in CASES if not c['room_cov'])                              # ... on either route


@pytest.mark.parametrize('case', CASES, ids=[rc.case_id(c) for c in CASES])
def test_emu_staged_step2_exact(make_engine, case):
    print(rc.check_staged(make_engine, **case))


@pytest.mark.parametrize('room_cov', [1, 0])
def test_emu_nan_stays_in_its_room_and_bin(make_engine, room_cov):
    rc.check_containment(make_engine, 8, 2, T=9, R=2, room_cov=room_cov)


@pytest.mark.parametrize('M,K,T', rc.reuse_cases(cut=True))
def test_emu_reuse_route_exact(make_engine, M, K, T):
    print(rc.check_reuse_exact(make_engine, M, K, T))


def test_emu_nan_beyond_a_rooms_own_frames_changes_nothing(make_engine):
    rc.check_nan_beyond(make_engine, 8, 2, T=9, frames=(9, 1, 6), room_cov=1)
    rc.check_nan_beyond(make_engine, 4, 6, T=17, frames=(17, 16, 1), room_cov=1)
