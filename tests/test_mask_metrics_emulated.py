"""The mask, VAD and level-statistics kernels (csrc/k_stft.h k_tf_mask / k_tf_mask_channel / k_mask_oracle, csrc/k_vad.h,
csrc/k_metrics.h) under the hipemu CPU emulator (no GPU): the checks of tests/test_gpu_mask_metrics.py through the same C ABI and Engine,
cut to the smallest shapes -- 100 elements per decade of the magnitude sweep, M = 2 and 3 for the per-channel masks, four oracle-mask
cases (every run boundary class once, both sizes, both pad modes), the short VAD lengths plus the 4096-hop signal once, one span per
bank beyond the two fw_snr banks.  The emulator divides and takes roots exactly, so what a 1-ulp instruction does on a tie is left to
the GPU file.  Test tooling only; the real runs are -m gpu.
Wall time: 25 s on an 8-core host."""
import pytest

import emu_build
import mask_metric_checks as mc
from disco_amd import _engines, _lib
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


def test_emu_every_accepted_mask_name(make_engine):
    print(mc.check_every_name(make_engine, n=1000))


def test_emu_magnitude_sweep(make_engine):
    print(mc.check_magnitude_sweep(make_engine, per_decade=100))


def test_emu_special_inputs(make_engine):
    mc.check_special_inputs(make_engine)


def test_emu_ibm_ties(make_engine):
    print(mc.check_ibm_ties(make_engine))


def test_emu_launch_geometry_and_batch_independence(make_engine):
    print(mc.check_geometry(make_engine))
    mc.check_mask_batch_independence(make_engine)


@pytest.mark.parametrize('M', (2, 3))
def test_emu_per_channel_masks_of_the_path(make_engine, M):
    for m, ref_mic, kind in mc.channel_cases((M,)):
        mc.check_channel_masks(make_engine, m, ref_mic, kind)


def test_emu_masks_z_with_compressed_rows(make_engine):
    mc.check_compressed_masks(make_engine, kinds=('irm1',))


def test_emu_oracle_masks_from_time_signals(make_engine):
    cases = mc.oracle_cases(cut=True)
    assert len(cases) == 4
    print([mc.check_oracle_case(make_engine, c, kinds=('irm1', 'iam2', 'ibm1') if i % 2 else ('irm2', 'iam1', 'ibm2')) for i, c in enumerate(cases)])


@pytest.mark.parametrize('n_fft', (512, 1024))
def test_emu_vad_mask(make_engine, n_fft):
    for L in mc.vad_lengths(n_fft, cut=True):
        mc.check_vad(make_engine, n_fft, L)


def test_emu_vad_mask_at_4096_hops_and_the_refusal_beyond(make_engine):
    mc.check_vad(make_engine, 512, 4096 * 256, alone=(3,))
    mc.check_vad_refusal(make_engine)


def test_emu_pair_stats(make_engine):
    print(mc.check_pair_stats(make_engine))


@pytest.mark.parametrize('bank', mc.BANKS)
def test_emu_band_stats(make_engine, bank):
    spans = mc.SPANS if isinstance(bank, str) else (mc.SPANS[1], mc.SPANS[2 + mc.BANKS.index(bank) % 4])
    for span in spans:
        print(bank, span, mc.check_band_case(make_engine, bank, span))


def test_emu_band_rows_alone(make_engine):
    mc.check_band_rows_alone(make_engine)
    mc.check_band_rows_alone(make_engine, bank=100, span=(257, 0, 257))


def test_emu_metrics_batch(emulated_package):
    print(mc.check_metrics_batch())
