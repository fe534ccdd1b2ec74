"""The reference's training set from rooms on the device (disco_theque/dataset_utils/post_generator.py PostGenerator): the mix at the drawn
SNR, the spectra of target, noise and mixture and the TF mask at every channel, and the files PostGenerator.save_data writes.

    post_process_rooms    post_generator.py:70-131    mix_sigs, array_stft and get_mask for R rooms at once, on the device
    write_post_dataset    post_generator.py:133-166   save_data's layout under <root>/<scene>/<case>/:

        wav_processed/<snr-dir>/target/<rir>_Ch-<c>.wav                              16-bit PCM (results_io.write_wav)
        wav_processed/<snr-dir>/{noise,mixture}/<rir>_<noise>_Ch-<c>.wav
        stft_processed/raw/<snr-dir>/target/<rir>_Ch-<c>.npy                          (F, T) complex64
        stft_processed/raw/<snr-dir>/{noise,mixture}/<rir>_<noise>_Ch-<c>.npy
        stft_processed/normed/abs/<snr-dir>/mixture/<rir>_<noise>_Ch-<c>.npy          (F, T) float32, np.abs of the raw file
        mask_processed/<snr-dir>/<rir>_<noise>_Ch-<c>.npy                             (F, T) float32
        log/snrs/dry/<snr-dir>/<rir>_<noise>.npy                                      (1,) the drawn SNR

    get_dset, get_directory_name    post_generator.py:58-68

Channels count from 1 over all microphones of the array, node after node.  dnn.utils.get_input_lists names these files for
dnn.data.SpectraBank.from_files; speech_enhancement.z_dataset.write_z_dataset adds the compressed signals under
<root>/<scene>/<case>/stft_z/<z_file>.  SpectraBank.from_rooms builds the same bank without any of the files.
The engine's arrays are frame-major (..., T, F); the files hold the reference's (F, T), cut to the room's own frames and samples."""
import os

import numpy as np

from .._engines import get_engine
from ..speech_enhancement import z_dataset
from ..speech_enhancement.results_io import write_wav
from .rooms import mix_rooms

DSETS = ('train', 'val', 'test')


def get_dset(rir, n_samples=None, nb_rir=0):
    """'train', 'val' or 'test' for RIR id `rir` (post_generator.py:58-64): n_samples = the sizes of the three sets in this order (default
    10000, 1000, 1000), ids count from 1 through the sets.  nb_rir: the run rir ... rir + nb_rir must stay inside the set, as the
    reference asserts.  ValueError where the reference's assertions fail."""
    edges = np.cumsum([10000, 1000, 1000] if n_samples is None else [int(v) for v in n_samples])
    if len(edges) != 3:
        raise ValueError('n_samples: the sizes of the train, val and test sets expected')
    if not 0 < rir < edges[-1]:
        raise ValueError('rir should be between 1 and {}'.format(str(edges[-1])))
    i_set = int(np.where(rir < edges)[0][0])
    if not rir + nb_rir < edges[i_set]:
        raise ValueError('First and last RIRs do not belong to the same set.')
    return DSETS[i_set]


def get_directory_name(snr_range):
    """[0, 6] -> '0-6' (post_generator.py:66-68); a list of ranges, [[0, 6]] or [[3, 6], [5, 15]], as get_input_lists and the z dataset take
    it -> '0-6', '3-6_5-15'."""
    if np.ndim(snr_range) == 1:
        return '{}-{}'.format(str(snr_range[0]), str(snr_range[1]))
    return z_dataset.get_directory_name(snr_range)


def post_process_rooms(tar_img, noi_img, snr, mics_per_node, lengths=None, mask_type='irm1', n_fft=512):
    """PostGenerator.post_process for R rooms on the device: tar_img (R, n_mic, L), noi_img (R, n_mic, Ln <= L), one snr (dB) per room.
    -> dict of device arrays: y, s, n (R, n_mic, L) -- the mix, target and scaled noise of mix_rooms --, Y, S, N (R, K, T, F, M) complex64, their
    spectra at EVERY channel, mask (R, K, T, F, M) float32, tf_mask(S, N) of `mask_type` at every channel; and of host data: frames (R,),
    lengths (R,), mics_per_node.  The spectra are Engine.stft of a node's M channels together, the groups the enhancement path transforms
    (channel pairs share a transform), so that at a reference microphone mask and mixture are bit for bit what step 1 of the path computes
    there.  lengths: as mix_rooms and Engine.set_lengths take them; frames at and beyond T_r = 1 + lengths[r] // hop are zero spectra."""
    y, s, n = mix_rooms(tar_img, noi_img, snr, mics_per_node, lengths=lengths)
    R, K, M, L = (int(v) for v in y.shape)
    eng = get_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft, mask=mask_type, pad_mode='reflect', ref_mic=0, mu=1.0, staged_step2=True)
    try:                                                                        # (a cached engine: the lengths do not outlive the call)
        if lengths is not None:
            eng.set_lengths(np.broadcast_to(np.asarray(lengths), (R,)))
        frames, lens = eng.frames, eng.lengths
        S, N, Y = (eng.stft(a.reshape(R * K, M, L)) for a in (s, n, y))
        mask = eng.tf_mask(S, N, type=mask_type)
    finally:
        if lengths is not None:
            eng.set_lengths(None)
    shape = (R, K, eng.T, eng.F, M)
    return dict(y=y.reshape(R, K * M, L), s=s.reshape(R, K * M, L), n=n.reshape(R, K * M, L), Y=Y.reshape(*shape), S=S.reshape(*shape),
                N=N.reshape(*shape), mask=mask.reshape(*shape), frames=frames, lengths=lens, mics_per_node=(M,) * K)


def _host(a):
    """A DevBuf, a tensor on any device or an array -> NumPy."""
    return np.asarray(a.cpu().numpy() if hasattr(a, 'cpu') else (a.numpy() if hasattr(a, 'numpy') else a))


def write_post_dataset(root, scene, case, rir_ids, noise, post, snr, snr_range, save_target=True, fs=16000):
    """PostGenerator.save_data (post_generator.py:133-166) for the R rooms of `post` (what post_process_rooms returned): the files listed at
    the top of this module under <root>/<scene>/<case>/, named by rir_ids (R,) and `noise`; snr: the SNR drawn for every room (a scalar or
    (R,)), logged as the reference logs it; snr_range: [lo, hi], naming <snr-dir>.  Room r is written with its own T_r frames and L_r
    samples.  save_target=False leaves the target's files out (they are the same for every noise).  A room whose SNR log exists is
    skipped, as the reference skips it (post_generator.py:75-76).  Returns the list of rooms written."""
    path_out = os.path.join(root, scene, case)
    snr_dir = get_directory_name(snr_range)
    for folder in (os.path.join('stft_processed', 'raw'), 'wav_processed'):
        for subfolder in ('target', 'noise', 'mixture'):
            os.makedirs(os.path.join(path_out, folder, snr_dir, subfolder), exist_ok=True)
    abs_dir = os.path.join(path_out, 'stft_processed', 'normed', 'abs', snr_dir, 'mixture')
    mask_dir = os.path.join(path_out, 'mask_processed', snr_dir)
    log_dir = os.path.join(path_out, 'log', 'snrs', 'dry', snr_dir)
    for d in (abs_dir, mask_dir, log_dir):
        os.makedirs(d, exist_ok=True)
    wavs = {k: _host(post[k]) for k in ('s', 'n', 'y')}
    R, n_mic, _ = wavs['y'].shape
    if len(rir_ids) != R:
        raise ValueError(f'{len(rir_ids)} rir_ids for {R} rooms')
    # (R, K, T, F, M) -> (R, K, M, F, T) -> (R, n_mic, F, T): the reference's orientation, channels node after node
    tf = {k: np.transpose(_host(post[k]), (0, 1, 4, 3, 2)) for k in ('S', 'N', 'Y', 'mask')}
    tf = {k: a.reshape(R, n_mic, a.shape[3], a.shape[4]) for k, a in tf.items()}
    snr = np.broadcast_to(np.asarray(snr, np.float64), (R,))
    written = []
    for r, rir in enumerate(rir_ids):
        log = os.path.join(log_dir, '{}_{}.npy'.format(str(rir), noise))
        if os.path.isfile(log):
            continue
        Lr, Tr = int(post['lengths'][r]), int(post['frames'][r])
        for i in range(n_mic):
            tar_name = '{}_Ch-{}'.format(str(rir), str(i + 1))
            name = '{}_{}_Ch-{}'.format(str(rir), noise, str(i + 1))
            if save_target:
                write_wav(os.path.join(path_out, 'wav_processed', snr_dir, 'target', tar_name + '.wav'), wavs['s'][r, i, :Lr], fs)
                np.save(os.path.join(path_out, 'stft_processed', 'raw', snr_dir, 'target', tar_name + '.npy'), np.ascontiguousarray(tf['S'][r, i, :, :Tr]))
            write_wav(os.path.join(path_out, 'wav_processed', snr_dir, 'noise', name + '.wav'), wavs['n'][r, i, :Lr], fs)
            write_wav(os.path.join(path_out, 'wav_processed', snr_dir, 'mixture', name + '.wav'), wavs['y'][r, i, :Lr], fs)
            mix = np.ascontiguousarray(tf['Y'][r, i, :, :Tr])
            np.save(os.path.join(path_out, 'stft_processed', 'raw', snr_dir, 'noise', name + '.npy'), np.ascontiguousarray(tf['N'][r, i, :, :Tr]))
            np.save(os.path.join(path_out, 'stft_processed', 'raw', snr_dir, 'mixture', name + '.npy'), mix)
            np.save(os.path.join(abs_dir, name + '.npy'), np.abs(mix))
            np.save(os.path.join(mask_dir, name + '.npy'), np.ascontiguousarray(tf['mask'][r, i, :, :Tr]))
        np.save(log, snr[r:r + 1])
        written.append(rir)
    return written
