"""The room pass (k_room_cov_dma), the split kernels that skip the step-1 block (k_cov_split_lds<M, KR, true>) and the re-use route of the
fused step 2 (k_step2_cov_fused<M, K, true>) on a real MI355X, pencil by pencil (tests/room_checks.py): the three producers of a pencil
that the solver assembles from two sets of partial blocks.  On exact scenes z must equal w_loc^H X bit for bit and every (room, node,
bin) matrix the exact sums -- bit for bit where the frame count is a power of two, inside 1.01 x 2^-23 otherwise --, with its leading block
the step-1 matrix bit for bit; the pending solve is held per pencil under both loaders of a two-block pencil.  All six shapes of the room
pass at 512 and 1024 points, all 24 of the split route, frame counts around the ring of the room pass and around the chunk boundaries of
the split route, one to three items per workgroup, per-room lengths, store_z = 0, containment of a NaN, and the Gaussian scene at 626
frames.  Lines starting with "room_routes" carry what the GPU showed."""
import pytest

import room_checks as rc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback
    return lambda **cfg: Engine(lib=lib, **cfg)


CASES = rc.staged_cases()


@pytest.mark.parametrize('case', CASES, ids=[rc.case_id(c) for c in CASES])
def test_staged_step2_exact(make_engine, case):
    res = rc.check_staged(make_engine, **case)
    for key, v in res.items():
        print('room_routes_solve', rc.case_id(case), key, tuple(f'{x:.3g}' for x in v))


@pytest.mark.parametrize('room_cov', [1, 0])
@pytest.mark.parametrize('M,K', [(8, 2), (4, 6), (8, 8)])
def test_nan_stays_in_its_room_and_bin(make_engine, M, K, room_cov):
    rc.check_containment(make_engine, M, K, T=17, R=2, room_cov=room_cov)


def test_nan_beyond_a_rooms_own_frames_changes_nothing(make_engine):
    """Every frame beyond a room's own T_r NaN in both X and mask; no output bit may change against the run with zeros there.  Step 1
    (k_cov_loc_f64<8>, k_cov<4, 0>) cuts its chunks at T_r and the room pass neither fetches nor weighs a frame beyond it and writes z = 0
    there (before this test existed both summed all T frames and turned every pencil of the shorter rooms into NaN)."""
    rc.check_nan_beyond(make_engine, 8, 2, T=17, frames=(17, 1, 9), room_cov=1)
    rc.check_nan_beyond(make_engine, 4, 6, T=33, frames=(33, 1, 17, 32), room_cov=1)


REUSE = rc.reuse_cases()


@pytest.mark.parametrize('M,K,T', REUSE, ids=[f'M{M}K{K}-T{T}' for M, K, T in REUSE])
def test_reuse_route_exact(make_engine, M, K, T):
    print('room_routes_reuse', (M, K, T), tuple(f'{x:.3g}' for x in rc.check_reuse_exact(make_engine, M, K, T)))


@pytest.mark.parametrize('room_cov', [1, 0])
@pytest.mark.parametrize('M,K', rc.FLOAT_SHAPES)
def test_float32_accumulation_at_626_frames(make_engine, M, K, room_cov):
    v = rc.check_float(make_engine, M, K, room_cov)
    print('room_routes_errors', (M, K, room_cov), {k: float(f'{x:.3g}') for k, x in v.items()})
