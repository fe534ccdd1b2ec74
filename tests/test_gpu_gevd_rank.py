"""Rank-R GEVD-MWF (disco_gevd_mwf, k_gevd_full.h) on a real MI355X: the reference's own outputs, the float64 closed form on the same
inputs for every P and route, rank 1 against the rank-1 solver, full rank without a gap, degenerate pencils, and the public surface."""
import os

import numpy as np
import pytest

import gevd_rank_checks as gr
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_reference_golden(make_engine, golden_dir):
    g = np.load(os.path.join(golden_dir, 'intern_filter_rank_ref.npz'))
    print(gr.check_against_golden(make_engine, g))


def test_every_size_and_rank_against_closed_form(make_engine):
    print(gr.check_sizes(make_engine, sizes=range(1, 17), batches=(1, 37)))


@pytest.mark.parametrize('P', [3, 4, 5, 8, 9, 16])
def test_large_ragged_and_2d_batches(make_engine, P):
    print(gr.check_batch_shapes(make_engine, P, n=100003))


def test_rank1_equals_rank1_solver(make_engine):
    print(gr.check_rank1_matches_r1(make_engine, sizes=range(1, 17)))


def test_full_rank_needs_no_gap(make_engine):
    print(gr.check_full_rank_no_gap(make_engine))


def test_degenerate_pencils(make_engine):
    gr.check_degenerate(make_engine)


def test_singular_noise_corank1_matches_oracle(make_engine):
    print(gr.check_singular_corank1_oracle(make_engine))


def test_negative_rank_is_refused(make_engine):
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    R = np.eye(3, dtype=np.complex64)[None]
    with pytest.raises(RuntimeError):
        eng.gevd_mwf(R, R, -1)


def test_intern_filter_surface(make_engine):
    gr.check_surface(make_engine)
