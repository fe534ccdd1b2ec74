"""BSS-eval SDR / SIR / SAR (disco_lag_corr, disco_bss_eval, csrc/k_bss.h) on a real MI355X at full size: mir_eval's 512-tap filter
(N = 1024 per two-source set) against the two float64 oracles of tests/bss_checks.py, closed forms, the permutation, batching and
chunking bit for bit, spans and mixed lengths, refusals, the BSS keys of room_results, and one C3-shaped room through the path."""
import pytest

import bss_checks as bc
from disco_amd import _lib

pytestmark = pytest.mark.gpu

FLOOR = ('floor1e-5',)


@pytest.fixture(scope='module', autouse=True)
def gfx950_library():
    _lib.load()          # raises if the gfx950 library is missing: no fallback


def test_spectra_flen512_against_dense():
    bc.check_against_oracle(bc.SPECTRA, 6000, 512, 2, oracle='dense', cond_max=1e7)


def test_noise_floor_1e5_flen512_against_dense():
    bc.check_against_oracle(FLOOR, 6000, 512, 2, oracle='dense', cond_max=1e11)


def test_spectra_flen512_full_length_against_gram():
    bc.check_against_oracle(bc.SPECTRA, 144000, 512, 2, oracle='gram', cond_max=1e7)


def test_noise_floor_1e5_flen512_full_length_against_gram():
    bc.check_against_oracle(FLOOR, 144000, 512, 2, oracle='gram', cond_max=1e11)


@pytest.mark.parametrize('nsrc,flen', [(1, 512), (3, 256), (4, 64), (3, 1), (2, 8)])
def test_other_source_counts_against_dense(nsrc, flen):
    bc.check_against_oracle(('white', 'butter8') + FLOOR, 5000, flen, nsrc, oracle='dense', cond_max=1e11)


def test_closed_forms():
    bc.check_closed_forms(16000, 512)


def test_permutation():
    bc.check_permutation(6000, 128)


def test_batching_bit_identical():
    bc.check_batching(6000, 512)


def test_start_stop_and_mixed_lengths():
    bc.check_start_stop_and_lengths(40000, 512)


def test_refusals():
    bc.check_refusals(6000)


def test_lag_corr():
    bc.check_lag_corr(50000)


def test_room_results_bss_keys(tmp_path):
    bc.check_room_results(512, tmp_path)


def test_c3_room_through_the_path():
    bc.check_c3_room_through_the_path()
