"""STOI (disco_stoi, csrc/k_stoi.h) on a real MI355X against the float64 yardstick of tests/stoi_checks.py: the compared cases, the
frame-count edges, the all-zero clean signal, batching / chunking / spans bit for bit, the STOI keys of room_results, one batch at
the span the reference scores (144 000 samples, 24 pairs) and one C3-shaped room through the path."""
import pytest

import stoi_checks as sc
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gfx950_library():
    _lib.load()          # raises if the gfx950 library is missing: no fallback


@pytest.mark.parametrize('fs,n', sc.CASES)
def test_against_yardstick(fs, n):
    sc.check_against_yardstick(fs, n)


def test_frame_count_edges():
    sc.check_frame_count_edges()


def test_all_zero_x():
    sc.check_all_zero_x()


def test_bit_identity():
    sc.check_bit_identity()


def test_device_resident():
    sc.check_device_resident()


def test_room_results_stoi_keys(tmp_path):
    sc.check_room_results(tmp_path)


def test_real_span_24_pairs_against_yardstick():
    sc.check_real_span()


def test_c3_room_through_the_path():
    sc.check_c3_room_through_the_path()
