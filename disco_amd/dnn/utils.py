"""The helpers of disco_theque/dnn/utils.py: `tf_mask` (:44-71, a verbatim duplicate of sigproc_utils.tf_mask in the reference, one
implementation here), the tensor `normalization` (:14-41), the file lists of the training set, `get_input_lists` (:74-140), and the frame
selection of the training loss, `get_loss_frames` / `get_x_for_loss` (:189-246).  The training and evaluation steps of that module are in
disco_amd/dnn/train.py."""
import os

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


NOISES = {'ssn': ['ssn'], 'it': ['it'], 'fs': ['fs'], 'noit': ['ssn', 'fs'], 'all': ['ssn', 'it', 'fs']}      # dnn/utils.py:115-120


def get_input_lists(path_to_data, rirs_to_get, scenes=None, snr_range=None, noise_to_get='ssn', ref_channel=1, z_sigs=None, z_file='oracle',
                    mics_per_node=(4, 4, 4, 4), rng=None):
    """The names of the files to train from (dnn/utils.py:74-140), as dataset_utils.post.write_post_dataset and
    speech_enhancement.z_dataset.write_z_dataset lay them out: a list of lists [K mixture lists, K lists per z signal, K mask lists], each
    with one file per RIR id of rirs_to_get -- what dnn.data.SpectraBank.from_files takes.  Per RIR: a scene drawn among `scenes` (a name or
    a list; None: 'random'), then a noise among those of noise_to_get ('ssn', 'it', 'fs'; 'noit': ssn or fs; 'all').  The draws come
    from `rng` (a numpy.random.Generator; None: a fresh one): the reference's global stream is not imitated.  snr_range: [lo, hi] or a list
    of such (None: [[0, 6]]); z_sigs: None, 'zs_hat', 'zn_hat' or a list; files are read under <path_to_data>/<scene>/train/, as the
    reference reads them.  The reference channel of node k is channel ref_channel + sum(mics_per_node[:k]) of the array, counted from 1: the
    reference writes ref_channel + n_nodes k, the same number for its four nodes of four microphones."""
    rng =np.random.default_rng() if rng is None else rng
    scenes = ['random'] if scenes is None else scenes
    scenes = list(scenes) if isinstance(scenes, (list, tuple)) else [scenes]
    if noise_to_get not in NOISES:
        raise ValueError(f'noise_to_get: one of {sorted(NOISES)} expected, got {noise_to_get!r}')
    noises = NOISES[noise_to_get]
    mpn = [int(m) for m in mics_per_node]
    n_nodes = len(mpn)
    if not 1 <= ref_channel <= min(mpn):
        raise ValueError(f'ref_channel {ref_channel}: 1 ... {min(mpn)} expected (the microphones of a node)')
    first = np.concatenate(([0], np.cumsum(mpn)[:-1]))
    z_names = [] if z_sigs is None else ([z_sigs] if isinstance(z_sigs, str) else list(z_sigs))
    snr_range = [[0, 6]] if snr_range is None else snr_range
    snr_range = [snr_range] if np.ndim(snr_range) == 1 else snr_range
    snr_dir = '_'.join('{}-{}'.format(str(r[0]), str(r[1])) for r in snr_range)
    out = [[] for _ in range(n_nodes * (2 + len(z_names)))]
    for rir in rirs_to_get:
        root = os.path.join(path_to_data, scenes[int(rng.integers(len(scenes)))], 'train', '')
        noise = noises[int(rng.integers(len(noises)))]
        path_y = os.path.join(root, 'stft_processed', 'normed', 'abs', snr_dir, 'mixture', '')
        path_m = os.path.join(root, 'mask_processed', snr_dir, '')
        for k in range(n_nodes):
            name = '{}_{}_Ch-{}.npy'.format(str(rir), noise, str(ref_channel + int(first[k])))
            out[k].append(path_y + name)
            out[len(out) - n_nodes + k].append(path_m + name)
            for i_sig, z_sig in enumerate(z_names):
                path_z = os.path.join(root, 'stft_z', z_file, 'normed', 'abs', snr_dir, z_sig, '')
                out[n_nodes * (1 + i_sig) + k].append(path_z + '{}_{}_Node-{}.npy'.format(str(rir), noise, str(k + 1)))
    return out


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
