"""The rank-R GEVD-MWF kernels (csrc/k_gevd_full.h) under the hipemu CPU emulator (no GPU), at small sizes: the same checks as
tests/test_gpu_gevd_rank.py through the same C ABI and Engine.  Test tooling only; the real runs are -m gpu."""
import os

import numpy as np
import pytest

import emu_build
import gevd_rank_checks as gr
from disco_amd import _engines, _lib
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_reference_golden(make_engine, golden_dir):
    g = np.load(os.path.join(golden_dir, 'intern_filter_rank_ref.npz'))
    print(gr.check_against_golden(make_engine, g))


def test_emu_every_size_and_rank(make_engine):
    print(gr.check_sizes(make_engine, sizes=range(1, 17), batches=(1, 5)))


@pytest.mark.parametrize('P', [3, 4, 5, 9])
def test_emu_ragged_and_2d_batches(make_engine, P):
    print(gr.check_batch_shapes(make_engine, P, n=301))


def test_emu_rank1_equals_rank1_solver(make_engine):
    print(gr.check_rank1_matches_r1(make_engine, sizes=range(1, 17), n=9))


def test_emu_full_rank_needs_no_gap(make_engine):
    print(gr.check_full_rank_no_gap(make_engine, n=5))


def test_emu_degenerate_pencils(make_engine):
    gr.check_degenerate(make_engine, n=9)


def test_emu_singular_noise_corank1(make_engine):
    print(gr.check_singular_corank1_oracle(make_engine))


def test_emu_negative_rank_is_refused(make_engine):
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    R = np.eye(3, dtype=np.complex64)[None]
    with pytest.raises(RuntimeError):
        eng.gevd_mwf(R, R, -1)


def test_emu_intern_filter_surface(make_engine, monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    try:
        gr.check_surface(make_engine)
    finally:
        _engines._cache.clear()
