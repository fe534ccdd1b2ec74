"""The online / adaptive MWF kernels (csrc/k_online.h) on a real MI355X at every pencil size, route and edge (tests/online_checks.py):
every (room, node, bin) problem and every frame against the float64 oracle, inside bars derived from the reference side alone.

Kernels launched here (api_online.hip's whole route table): k_online_mwf_thread<1>, <2>, <3>, <4>, <5>, <6>, <7> with packed-float32
and with float64 squarings; k_online_mwf<5>, <6>, <7> ("solve_thread" = 0), k_online_mwf<8> (8 lanes per problem) and k_online_mwf<9>,
<10>, <11>, <12>, <13>, <14>, <15>, <16> (16 lanes per problem).  Lines starting with "online " carry what the GPU showed."""
import pytest

import online_checks as oc
import parity_checks as pc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('variant', ['d1', 'd1e-3'])
def test_every_size_and_route_against_oracle(make_engine, variant):
    """Check 1: P = 1 .. 16 in the step-1 form, every step-2 shape, every route; init_diag = 1 and the shipped 1e-3."""
    print('online_sizes_errors', variant, oc.check_sizes(make_engine, variant))


def test_update_schedule(make_engine):
    """Check 2: update_every in {1, 2, 3, T - 1, T, T + 5} on the thread, 8-lane and 16-lane kernels, frame by frame."""
    print(oc.check_schedule(make_engine))


def test_row_order_and_z_layout(make_engine):
    """Check 3: node shards at every k0 of K = 6 (P = 7, both routes) and K = 9 (P = 16); rank-major z blocks bit-identical."""
    print(oc.check_row_order(make_engine))


# check 4: (M, K) -> P2 = M + K - 1 = 5, 6, 7 through the group kernel ("solve_thread" = 0; step 1 at M = 5 runs it too) and every size it
# always serves; update_every > 1 so that updates fall inside chunks; ragged, one-call, interleaved and hop-by-hop chunkings
@pytest.mark.parametrize('M,K,U,opts', [(3, 3, 3, {'solve_thread': 0}), (5, 2, 2, {'solve_thread': 0}), (4, 4, 3, {'solve_thread': 0}),
                                        (4, 5, 3, None), (8, 3, 2, None), (6, 6, 3, None), (8, 5, 2, None), (8, 6, 3, None),
                                        (8, 7, 2, None), (8, 8, 3, None), (8, 9, 2, None)])
def test_group_kernel_stream_equals_whole_clip(make_engine, M, K, U, opts):
    """Chunked stream == whole clip, bit for bit, on k_online_mwf<P> at P2 = 5, 6, 7, 8, 10 .. 16 (8 and 9: test_gpu_parity.py): the
    resumable state keeps lower triangles only, so both triangles must have been rounded identically."""
    print(pc.check_online_stream(make_engine, R=2, K=K, M=M, L=6144, n_fft=512, update_every=U, options=opts))


def test_mask_and_parameter_edges(make_engine):
    """Check 5: mask == 0, mask == 1 (40 frames), masks of exactly 0 and 1, lambda 0 and 0.999, mu 0.3 and 10."""
    print(oc.check_edges(make_engine))


def test_argument_refusals(make_engine):
    oc.check_refusals(make_engine)


def test_nonfinite_input_stays_where_it_is(make_engine):
    """Check 6: a NaN / an inf in X, a NaN in one remote z: every other problem and every earlier frame bit-identical."""
    oc.check_nonfinite(make_engine)


def test_thread_route_against_group_route(make_engine):
    """Check 7: P = 5, 6, 7, the two routes on the same inputs."""
    print(oc.check_routes(make_engine))
