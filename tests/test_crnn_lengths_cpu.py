"""CRNN.predict_masks(..., frames=...) on the CPU in float64: items of different lengths in one batch, each against the reference's own
evaluation order on the truncated sequence (tests/crnn_length_checks.py).  No GPU, no kernel."""
import pytest
import torch

import crnn_length_checks as cl


@pytest.mark.parametrize('n_ch', [1, 3])
@pytest.mark.parametrize('ftp', ['mid', 'last'])
def test_predict_masks_frames_vs_windowed_float64(n_ch, ftp):
    print(cl.check_predict_masks_frames('cpu', n_ch, ftp, torch.float64, 1e-12))


def test_predict_masks_uniform_batch_and_refusals():
    assert cl.check_predict_masks_uniform_and_refusals('cpu', torch.float64, 1e-12)


def test_prototypes_of_the_three_entries():
    from disco_amd import _lib
    assert {'disco_crnn_features_rooms', 'disco_crnn_windows_rooms', 'disco_crnn_expand_rows'} <= set(_lib.PROTOTYPES)
