"""The helpers of disco_theque/dnn/utils.py: `tf_mask` (:44-71, a verbatim duplicate of sigproc_utils.tf_mask in the reference, one
implementation here), the tensor `normalization` (:14-41), and the frame selection of the training loss, `get_loss_frames` /
`get_x_for_loss` (:189-246).  The training and evaluation steps of that module are in disco_amd/dnn/train.py."""
import numpy as np
import torch

from ..sigproc_utils import tf_mask  # noqa: F401


def normalization(x, norm_type=None, axis=0):
    """Normalise tensor `x` along `axis` (dnn/utils.py:14-41): 'scale_to_unit_norm' (divide by the 2-norm), 'scale_to_1'
    (divide by the maximum), 'center_and_scale' (subtract the mean, divide by the unbiased standard deviation -- torch.std's
    default, as the reference calls it); anything else returns `x` unchanged, as the reference does.  Stays on x's device."""
    if norm_type == 'scale_to_unit_norm':
        return x / torch.linalg.vector_norm(x, dim=axis, keepdim=True)
    if norm_type == 'scale_to_1':
        return x / torch.amax(x, dim=axis, keepdim=True)
    if norm_type == 'center_and_scale':
        x = x - torch.mean(x, dim=axis, keepdim=True)
        return x / torch.std(x, dim=axis, keepdim=True)
    return x


def get_loss_frames(win_len, part):
    """(first, last + 1) of the frames of a `win_len`-frame window the loss looks at (dnn/utils.py:189-209): 'all', 'mid' (frame
    int(ceil(win_len) / 2), as the reference writes it), 'last', or an integer frame."""
    if part == 'all':
        return 0, win_len
    if part == 'mid':
        first = int(np.ceil(win_len) / 2)
    elif part == 'last':
        first = win_len - 1
    elif isinstance(part, (int, np.integer)) and not isinstance(part, bool):
        first = int(part)
    else:
        raise ValueError("Unknown argument value {}. It should be either 'all', 'mid' or 'last'.".format(part))
    return first, first + 1


def get_x_for_loss(x, part, model=None, model_output=1, n_freq=257):
    """The frames of `x` that the loss compares (dnn/utils.py:212-246): x (B, W, F) or (B, C, W, F) (channel 0 is taken);
    model given: its get_loss_frames(part)[model_output] (0: frames of the input / label, 1: of the output), else those of
    get_loss_frames over x's own length; the first n_freq features; squeezed, as the reference returns it."""
    if model is None:
        ff, lf = get_loss_frames(x.shape[-2], part)
    else:
        ff, lf = model.get_loss_frames(part)[model_output]
    if x.dim() == 3:
        x_out = torch.squeeze(x[:, ff:lf, :])
    elif x.dim() == 4:
        x_out = torch.squeeze(x[:, 0, ff:lf, :])
    else:
        raise NotImplementedError('Unexpected case')
    return torch.squeeze(x_out[..., :n_freq])
