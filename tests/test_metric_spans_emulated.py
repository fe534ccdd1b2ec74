"""The per-signal spans of the metric kernels (csrc/k_metrics.h, csrc/k_bss.h) and results_io.batch_results under the hipemu CPU emulator
(no GPU): the same checks as tests/test_gpu_metric_spans.py through the same C ABI, Engine and disco_amd.metrics, with a 64-tap BSS
filter in batch_results.  Test tooling only; the real runs are -m gpu.  The room through the whole path is left to the GPU file."""
import pytest

import emu_build
import span_checks as sp
from disco_amd import _engines, _lib


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


def test_emu_pair_stats_spans(emulated_package):
    sp.check_pair_stats()


@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('bank', ['wide18', 'narrow14'])
def test_emu_band_stats_spans(emulated_package, bank, gated):
    sp.check_band_stats(bank, gated)


def test_emu_lag_corr_spans(emulated_package):
    sp.check_lag_corr()


def test_emu_bss_estimates(emulated_package):
    sp.check_bss_estimates()


def test_emu_bss_eval_spans(emulated_package):
    sp.check_bss_eval_spans()


def test_emu_metrics_array_stop(emulated_package):
    sp.check_metrics_array_stop()


def test_emu_batch_results(emulated_package, tmp_path):
    sp.check_batch_results(64, tmp_path)


def test_emu_batch_results_zero_reference(emulated_package):
    sp.check_batch_zero_reference()
