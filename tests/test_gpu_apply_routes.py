"""The filter-and-sum and inverse-transform kernels on a real MI355X, output by output, on every route (tests/apply_checks.py): every
instantiation that disco_apply, disco_step2_apply_fused, disco_step2_apply_istft_fused, disco_apply_istft_fused and disco_istft can
reach.  Filter outputs on exact scenes must equal the float64 sums bit for bit, every (room, node, frame, bin), for conj_w = 1 and 0;
then the launch geometry, node shards and rank-major z blocks against the unsharded run, per-room lengths, containment of a NaN, the
documented refusals, X beyond 2^31 elements.  The inverse transforms are held per (room, node, hop segment) to 4 x the distance of a
float32 NumPy / SciPy restatement from the float64 oracle: run boundaries at 2, 3, 4, 64 and the heuristic's frame pairs per run, odd
and even frame counts, tails, clips of 1 .. 3 frames, per-room lengths, the fused kernels against the staged calls, a NaN frame.

Kernels launched here: profiles/apply_routes_kernels.txt (a kernel trace of this file; tests/test_apply_routes_cpu.py holds it
against the route table).  Lines starting with "apply_routes" carry what the GPU showed (profiles/apply_routes_errors.json).
18 tests, 7 s on an MI355X (the 2 x 17 GB of the large-offset cases included)."""
import pytest

import apply_checks as ac
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('family', ['k_apply<', 'k_apply_m<', 'k_apply_mq<'])
def test_disco_apply_every_reachable_instantiation_exact(make_engine, family):
    """R = 2, F = 257 (four full tiles and the one-lane tile) or 513, T from {1, 2, 3, 9}, conj_w = 1 and 0."""
    cases = [c for c in ac.apply_cases() if ac.route(c['M'], c['K'], c['n_fft'], 'apply', step2=c['step2'])[0].startswith(family)]
    assert cases
    print('apply_routes', family, len(cases), 'cases:', ac.check_apply_cases(make_engine, cases))


def test_disco_apply_every_default_frame_count(make_engine):
    for M, K in ((2, 3), (3, 8), (8, 4), (4, 7), (2, 18)):
        for T in ac.T_DEFAULT:
            ac.check_apply(make_engine, M, K, T=T)


def test_step2_apply_fused_all_36_shapes_exact(make_engine):
    """yf and z_out; T = 9 (two full groups of 4 frames and one of 1) and, at 1024 points, 3."""
    for i, (M, K) in enumerate(ac.fused_shapes()):
        ac.check_step2_fused(make_engine, M, K, T=(9, 3, 2, 1)[i % 4] if i % 5 else 9)
    for M, K in ((1, 2), (2, 3), (4, 4), (1, 8), (7, 2), (8, 1)):
        ac.check_step2_fused(make_engine, M, K, 1024, T=3)


def test_apply_istft_fused_spectra_all_18_instantiations_exact(make_engine):
    for i, (n_fft, M, K) in enumerate(ac.wide_shapes()):
        ac.check_wide_yf(make_engine, n_fft, M, K, T=ac.T_DEFAULT[i % 4], pairs=(0, 2, 3)[i % 3])


def test_heads_and_residuals_exact(make_engine):
    ac.check_heads_and_residuals(make_engine)


def test_launch_geometry_of_disco_apply(make_engine):
    print(ac.check_geometry_apply(make_engine))


def test_launch_geometry_of_step2_apply_fused(make_engine):
    print(ac.check_geometry_fused(make_engine))


def test_node_shards_and_z_blocks(make_engine):
    print(ac.check_shards(make_engine))


def test_per_room_lengths(make_engine):
    print(ac.check_lengths(make_engine))


def test_nan_stays_where_the_algebra_puts_it(make_engine):
    ac.check_nonfinite(make_engine)


def test_refusals_leave_the_context_usable(make_engine):
    ac.check_refusals(make_engine)


def test_x_beyond_2_31_elements(make_engine):
    """k_apply and k_apply_mq on 17 GB of spectra generated on the device; first and last room exact on the host."""
    print('apply_routes_huge', ac.check_huge(make_engine, 'cuda'))


@pytest.mark.parametrize('entry', ['istft', 'step2_istft', 'apply_istft'])
def test_inverse_transforms_per_hop_segment(make_engine, entry):
    """Worst and median ratio, over every live (room, node, hop segment), of the kernel's distance from the float64 oracle to the float32
    restatement's (the bar is 4)."""
    import json
    cases = [c for c in ac.istft_cases() if c['entry'] == entry]
    for fam, v in ac.check_istft_cases(make_engine, cases).items():
        print('apply_routes_errors', json.dumps({fam: v}))


def test_nan_frame_stays_within_two_frames(make_engine):
    ac.check_istft_nonfinite(make_engine)
