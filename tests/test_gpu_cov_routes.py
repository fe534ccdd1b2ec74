"""The masked-covariance kernels on a real MI355X, pencil by pencil, on every route and shape (tests/cov_checks.py): every
instantiation that disco_cov_masked and disco_step2_cov_fused can reach, on scenes whose sums are exact, so that every (room, node, bin)
matrix must equal the float64 sums -- bit for bit where the frame count is a power of two, inside the derived 1.01 x 2^-23 of the
mean's two roundings otherwise; then the launch geometry (chunks of exactly 64, 65 and 129 frames, 626 frames in one chunk, frame
counts below the chunk count), node shards and rank-major z blocks, per-room lengths, containment of a NaN, the documented refusals,
X beyond 2^31 elements, the solvers' own loaders of the partial blocks (disco_gevd_mwf_r1_pending at 1, 2, 3, 5 and 8 chunks through all
four solver files), z_out and the solve of the re-use route, and what cannot be exact: the staged families on a Gaussian scene at 626
frames in one chunk, and disco_stft_cov_fused end to end against the complex128 transform.

Kernels launched here: profiles/cov_routes_kernels.txt (a kernel trace of this file; tests/test_cov_routes_cpu.py holds it against the
route table).  23 tests, 38 s on an MI355X.  Lines starting with "cov_routes" carry what the GPU showed (profiles/cov_routes_errors.json)."""
import pytest

import cov_checks as cc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('family', cc.CASE_FAMILIES)
def test_every_reachable_instantiation_exact(make_engine, family):
    """64 frames (a power of two: bit equality) in the heuristic's 8 chunks of 8."""
    cases = [c for c in cc.exact_cases() if cc.family_of(c) == family]
    assert cases
    print('cov_routes', family, len(cases), 'cases:', cc.check_exact_cases(make_engine, cases, T=64))


@pytest.mark.parametrize('family', sorted(cc.FAMILIES) + ['k_step2_cov_fused'])
def test_launch_geometry(make_engine, family):
    print(cc.check_geometry(make_engine, families=(family,)))


def test_default_heuristic_picks_one_chunk(make_engine):
    cc.check_default_single_chunk(make_engine)


def test_node_shards_and_z_blocks(make_engine):
    print(cc.check_shards(make_engine))


def test_per_room_lengths(make_engine):
    print(cc.check_lengths(make_engine))


def test_nan_stays_in_its_pencils(make_engine):
    cc.check_nonfinite(make_engine)


def test_refusals_leave_the_context_usable(make_engine):
    cc.check_refusals(make_engine)


def test_pending_solves_read_every_partial_block(make_engine):
    """Worst per-pencil distance from the float64 oracle, share of pencils at the 2e-6 floor bar, median reference-side distance, the
    solver whose loader read the blocks; identical at 1, 2, 3, 5 and 8 chunks (asserted)."""
    for key, v in cc.check_pending(make_engine).items():
        print('cov_routes_pending', key, tuple(f'{x:.3g}' for x in v[:3]), v[3])


def test_reuse_route_every_shape(make_engine):
    """All 28 shapes: z_out and, per pencil, the solve assembled from both sets of partial blocks."""
    for key, v in cc.check_reuse(make_engine, T=64).items():
        print('cov_routes_reuse', key, tuple(f'{x:.3g}' for x in v))


def test_stft_cov_fused_against_the_float64_transform(make_engine):
    """Every k_stft_cov<n_fft, M>, the staged pair at 1024 points and 7, 8 microphones, both pad modes, runs of 8, 40, 79, 80 and 400
    frames per wave, a last workgroup with empty waves, clips of 2 and 3 frames, per-room lengths."""
    for cid, v in cc.check_stft_cov(make_engine).items():
        print('cov_routes_stft', cid, {k: float(f'{x:.3g}') for k, x in v.items()})


def test_float32_accumulation_at_the_production_chunk_length(make_engine):
    """626 frames in one chunk on the Gaussian scene: every pencil inside 4 x the reference-side distance (cov_checks.FLOAT_DIST)."""
    for fam, v in cc.check_float(make_engine).items():
        print('cov_routes_errors', fam, {k: float(f'{x:.3g}') for k, x in v.items()})


def test_x_beyond_2_31_elements(make_engine):
    """k_cov and k_cov_big on 17 GB of spectra generated on the device; first and last room exact on the host."""
    print('cov_routes_huge', cc.check_huge(make_engine, 'cuda'))
