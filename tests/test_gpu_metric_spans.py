"""The per-signal spans of the metric kernels (disco_pair_stats_spans, disco_band_stats_spans, disco_lag_corr_spans, disco_bss_eval_spans,
disco_bss_estimates), `stop` arrays in disco_amd.metrics and results_io.batch_results on a real MI355X (tests/span_checks.py): every
signal of a batch of different clip lengths, NaN past its own end, against the scalar call on that signal alone, bit for bit; a batch
of three rooms against room_results per room; and three rooms through the path, device-resident from the samples to the figures."""
import pytest

import span_checks as sp
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def gfx950_library():
    _lib.load()          # raises if the gfx950 library is missing: no fallback


def test_pair_stats_spans():
    sp.check_pair_stats()


@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('bank', ['wide18', 'narrow14'])
def test_band_stats_spans(bank, gated):
    sp.check_band_stats(bank, gated)


def test_lag_corr_spans():
    sp.check_lag_corr()


def test_bss_estimates():
    sp.check_bss_estimates()


def test_bss_eval_spans():
    sp.check_bss_eval_spans()


def test_metrics_array_stop():
    sp.check_metrics_array_stop()


def test_batch_results(tmp_path):
    sp.check_batch_results(512, tmp_path)


def test_batch_results_zero_reference():
    sp.check_batch_zero_reference()


def test_three_rooms_through_the_path():
    lib = _lib.load()
    sp.check_through_the_path(lambda **cfg: Engine(lib=lib, **cfg))
