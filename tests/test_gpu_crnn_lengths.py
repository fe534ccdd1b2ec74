"""CRNN-mask batches whose rooms differ in clip length, on the MI355X: the three helper kernels, predict_masks(..., frames=...) in float32
against the float64 network, and both routes per room against the float64 oracle and against the room run alone
(tests/crnn_length_checks.py)."""
import pytest

import crnn_length_checks as cl
from disco_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    import torch
    torch.cuda.set_device(0)
    return 'cuda:0'


@pytest.mark.parametrize('shape,frame_sets', [((3, 3, 2, 9, 17), ((9, 1, 4),)), ((2, 4, 4, 40, 257), ((40, 1), (20, 40)))])
def test_crnn_features_rooms(dev, shape, frame_sets):
    print(cl.check_features_rooms(_lib.load(), dev, *shape, frame_sets))


def test_crnn_windows_rooms(dev):
    assert cl.check_windows_rooms(_lib.load(), dev)


def test_crnn_expand_rows(dev):
    assert cl.check_expand_rows(_lib.load(), dev)


def test_windows_and_expand_beyond_one_grid_pass(dev):
    print('N / (B T) =', cl.check_beyond_one_grid_pass(_lib.load(), dev))


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('n_ch', [1, 3])
@pytest.mark.parametrize('ftp', ['mid', 'last'])
def test_predict_masks_frames_float32_vs_float64(dev, n_ch, ftp, fused):
    """2e-5: what test_predict_masks_float32_vs_float64_production_shape holds float32 predict_masks to (library GEMMs and convolutions of
    another shape), on output weights of ordinary scale as there (crnn_length_checks.rand_model, out_gain)."""
    import torch
    print(cl.check_predict_masks_frames(dev, n_ch, ftp, torch.float32, 2e-5, fused=fused, out_gain=1.0))


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('n_ch', [1, 3])
@pytest.mark.parametrize('ftp', ['mid', 'last'])
def test_predict_masks_frames_float32_vs_item_alone_x40(dev, n_ch, ftp, fused):
    """The x 40 output weights of the whole-path recipe, float32 on both sides: predict_masks(frames=)[b, :T_b] against the rectangular
    predict_masks of item b alone at 2e-5 (two float32 evaluations of one network at different batch shapes, the bar of the in-loop
    batch-against-alone check).  Against float64 the x 40 network is only held to 1e-3 here: that distance is the rectangular path's as well."""
    import torch
    print(cl.check_predict_masks_frames(dev, n_ch, ftp, torch.float32, 1e-3, fused=fused, alone_tol=2e-5)[1])


def test_predict_masks_uniform_batch_and_refusals_on_gpu(dev):
    import torch
    assert cl.check_predict_masks_uniform_and_refusals(dev, torch.float32, 2e-5, out_gain=1.0)


@pytest.mark.parametrize('K,M,two_models', [(3, 2, True), (3, 2, False), (4, 4, True), (4, 4, False), (1, 4, True)])
def test_in_loop_mixed_lengths_vs_oracle_and_alone(dev, K, M, two_models):
    cl.check_in_loop(_lib.load(), K, M, two_models)


@pytest.mark.parametrize('variant', sorted(cl.SURFACE_VARIANTS))
def test_offline_tango_rooms_with_crnn_masks(dev, variant):
    cl.check_surface(dev, variant)
