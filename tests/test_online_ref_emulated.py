"""Scoring the online mode under the hipemu CPU emulator (no GPU): the checks of tests/test_gpu_online_ref.py through the same C ABI
and Engine, cut to one room and a prefix of the frames as tests/test_online_sizes_emulated.py is (the walk is causal and rooms are
independent, so a prefix is a case of its own; its bars are measured on the spot, tests/online_ref_checks.py).  Test tooling only; the
real runs are -m gpu."""
import pytest

import emu_build
import online_checks as oc
import online_ref_checks as rc
from disco_amd import _engines, _lib
from disco_amd.engine import Engine

CUT = (1, 8)


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_every_size_and_route(make_engine):
    """Every instantiated companion kernel: k_online_mwf_thread_ref<1> .. <7> (both squarings), k_online_mwf_ref<5> .. <16>."""
    print(rc.check_sizes(make_engine, 'd1', step2=((1, 2), (2, 6), (8, 2), (8, 9)), cut=CUT))


def test_emu_sizes_at_the_shipped_init_diag(make_engine):
    print(rc.check_sizes(make_engine, 'd1e-3', step1=(1, 4, 7, 8, 16), step2=((2, 6),), cut=CUT))


def test_emu_filter_in_force(make_engine):
    """All twelve frames: T - 1, T and T + 5 keep their meaning."""
    print(rc.check_schedule(make_engine, cut=(1, oc.T_SCHED)))


def test_emu_row_order_and_layouts(make_engine):
    print(rc.check_row_order(make_engine, cut=CUT, every_k0=False))


def test_emu_one_companion(make_engine):
    rc.check_one_companion(make_engine, cut=CUT)


def test_emu_companions_do_not_feed_the_recursion(make_engine):
    rc.check_containment(make_engine, step1=(4, 8), step2=((2, 6), (8, 9)), cut=CUT)


def test_emu_argument_refusals(make_engine):
    rc.check_refusals(make_engine)


@pytest.mark.parametrize('K,M,opts', [(3, 2, None), (4, 4, {'solve_thread': 0})])
def test_emu_whole_path(make_engine, K, M, opts):
    """One room of six frames: the emulator pays per launch and per block."""
    rc.check_whole_path(make_engine, R=1, K=K, M=M, L=1280, options=opts)


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


def test_emu_surface(emulated_package):
    """online_tango_batched / online_tango on the emulator library: keys, shapes and dtypes of offline_tango_batched, one room against
    the batch, masks= against vads."""
    rc.check_surface(L=1280)
