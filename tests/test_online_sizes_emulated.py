"""The online / adaptive MWF kernels (csrc/k_online.h) under the hipemu CPU emulator (no GPU): the checks of
tests/test_gpu_online_sizes.py through the same C ABI and Engine, cut to one room and a prefix of the frames (the walk is causal and
rooms are independent, so a prefix is a case of its own; its bar is measured on the spot, tests/online_checks.py).  One room of 257 bins
is still no multiple of the 16 / 4 problems of a block: the dead-group path runs.  Test tooling only; the real runs are -m gpu.
Wall time: 210 s on an 8-core host, in one run of the whole CPU suite where tests/test_kernels_emulated_wide.py took 519 s."""
import pytest

import emu_build
import online_checks as oc
import parity_checks as pc
from disco_amd.engine import Engine

CUT = (1, 8)


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_every_size_and_route_against_oracle(make_engine):
    """Every instantiated kernel: k_online_mwf_thread<1> .. <7> (both squarings), k_online_mwf<5> .. <16>; five step-2 shapes."""
    print(oc.check_sizes(make_engine, 'd1', step2=((1, 2), (2, 6), (4, 5), (8, 2), (8, 9)), cut=CUT))


def test_emu_sizes_at_the_shipped_init_diag(make_engine):
    print(oc.check_sizes(make_engine, 'd1e-3', step1=(1, 4, 5, 7, 8, 9, 16), step2=((2, 6),), cut=CUT))


def test_emu_update_schedule(make_engine):
    """All twelve frames: T - 1, T and T + 5 keep their meaning."""
    print(oc.check_schedule(make_engine, cut=(1, oc.T_SCHED)))


def test_emu_row_order_and_z_layout(make_engine):
    print(oc.check_row_order(make_engine, cut=CUT, every_k0=False))


@pytest.mark.parametrize('M,K,U,opts', [(3, 3, 3, {'solve_thread': 0}), (4, 4, 2, {'solve_thread': 0}), (4, 5, 3, None), (8, 2, 2, None),
                                        (8, 9, 3, None)])
def test_emu_group_kernel_stream_equals_whole_clip(make_engine, M, K, U, opts):
    """k_online_mwf<P> resumed from its triangular state at P2 = 5, 7, 8, 9, 16 (g++ makes its own contraction choices: whether the
    gfx950 build rounds both triangles alike is what the GPU test shows).  Four hops: the emulator pays per launch and per block, and the
    hop-by-hop chunking is many small launches."""
    print(pc.check_online_stream(make_engine, R=1, K=K, M=M, L=1024, n_fft=512, update_every=U, chunks=(3, 1, 2), options=opts))


def test_emu_mask_and_parameter_edges(make_engine):
    print(oc.check_edges(make_engine, cut=(1, 8)))


def test_emu_argument_refusals(make_engine):
    oc.check_refusals(make_engine)


def test_emu_nonfinite_input_stays_where_it_is(make_engine):
    oc.check_nonfinite(make_engine, cut=CUT)


def test_emu_thread_route_against_group_route(make_engine):
    print(oc.check_routes(make_engine, cut=CUT))
