"""Networks whose step-2 pencils exceed 16 channels (17 <= P = M + K - 1 <= 32) on a real MI355X: the wide covariance kernel
(csrc/k_cov_wide.h), the wide rank-1 solver (csrc/k_solve_wide.h) from full matrices and from partial sums, the filter, the whole path,
the reference-output path, the iterated path, intern_filter, the reference's own outputs (tests/golden/tango_ref_wide.npz) and the
refusals beyond the limits."""
import numpy as np
import pytest

import parity_checks as pc
import wide_checks as wc
from disco_amd import _lib
from disco_amd.engine import DiscoError, Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_wide_solver_full_matrices(make_engine):
    print(wc.check_solver_full(make_engine, sizes=range(17, 33), n=37))


def test_wide_solver_indefinite(make_engine):
    print(pc.check_solver_indefinite(make_engine, sizes=range(17, 33)))


def test_wide_solver_small_gap(make_engine):
    print(wc.check_solver_small_gap(make_engine))


def test_wide_solver_nan_neighbours(make_engine):
    assert wc.check_solver_nan_neighbours(make_engine, P=20, n=11)
    assert wc.check_solver_nan_neighbours(make_engine, P=32, n=9)


@pytest.mark.parametrize('K,M', [(16, 2), (10, 8), (25, 8), (17, 1)])
def test_wide_solver_from_partials(make_engine, K, M):
    print(wc.check_solver_from_partials(make_engine, K, M, R=2))


@pytest.mark.parametrize('K,M', [(16, 2), (10, 8), (25, 8)])
def test_wide_staged_cov_solve_apply(make_engine, K, M):
    print(wc.check_staged(make_engine, K, M, R=2))


@pytest.mark.parametrize('R,K,M', [(2, 16, 2), (2, 16, 4), (1, 25, 8)])
def test_wide_end_to_end(make_engine, R, K, M):
    L = (4 * (M + K - 1) + 4) * 256
    print(wc.check_end_to_end(make_engine, R, K, M, L))


def test_wide_reference_outputs_every_mode(make_engine):
    print(wc.check_reference_outputs_oracle(make_engine, K=16, M=2, L=(4 * 17 + 4) * 256))


def test_wide_iterated(make_engine):
    assert pc.check_iterated_outputs(make_engine, K=16, M=2, L=(4 * 17 + 4) * 256, n_fft=512, iters=2)


@pytest.mark.parametrize('P', [20, 32])
def test_wide_intern_filter(P):
    assert wc.check_intern_filter(P)


def test_wide_refusals(make_engine):
    assert wc.check_refusals(make_engine, DiscoError)


@pytest.mark.parametrize('scene', wc.WIDE_SCENES, ids=[s[0] for s in wc.WIDE_SCENES])
def test_wide_offline_tango_vs_reference(golden_dir, scene):
    from disco_amd.speech_enhancement.tango import offline_tango
    print(wc.check_reference_wide(offline_tango, golden_dir, scene))
