"""ESTOI (disco_estoi, disco_estoi_bands, csrc/k_estoi.h) on a real MI355X against the float64 yardstick of tests/estoi_checks.py: the
compared cases, the last stage alone on exact and degenerate envelopes, the frame-count edges, the all-zero clean signal, batching /
chunking / spans bit for bit (and STOI untouched by an ESTOI call), the ESTOI keys of room_results and batch_results, the refusals, and
one batch at the span the reference scores (144 000 samples, 24 pairs)."""
import pytest

import estoi_checks as ec
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gfx950_library():
    _lib.load()          # raises if the gfx950 library is missing: no fallback


@pytest.mark.parametrize('fs,n', ec.CASES)
def test_against_yardstick(fs, n):
    ec.check_against_yardstick(fs, n)


def test_bands_frame_counts():
    ec.check_bands_frame_counts()


def test_bands_degenerate():
    ec.check_bands_degenerate()


def test_frame_count_edges():
    ec.check_frame_count_edges()


def test_all_zero_x_and_identity():
    ec.check_all_zero_x_and_identity()


def test_bit_identity():
    ec.check_bit_identity()


def test_device_resident():
    ec.check_device_resident()


def test_room_results_estoi_keys(tmp_path):
    ec.check_room_results(tmp_path)


def test_batch_results_estoi_keys():
    ec.check_batch_results()


def test_surface():
    ec.check_surface()


def test_real_span_24_pairs_against_yardstick():
    ec.check_real_span()
