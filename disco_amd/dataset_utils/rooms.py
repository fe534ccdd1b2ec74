"""snr_at_mics, simulate_rooms, mix_rooms: the steps between a dry source and a batch of rooms for offline_tango_batched.

    snr_at_mics      convolve_signals.py:170-213    SNR per microphone (fw_snr mean), per node, and the reference's node-to-node difference
    simulate_rooms   convolve_signals.py:255-273    R rooms at once: noise level, RIRs, images, image VADs, SNRs, the acceptance rule
    mix_rooms        post_generator.py:99-115       the mix at one drawn SNR per room
    reverb_at_mics   metrics.py:176-208             how reverberant the rooms came out: DRR and SRR at every microphone

The signals stay on the device between the steps (DevBuf); the figures (SNRs, flags) are NumPy.  Nothing is drawn and nothing is redrawn
here: room geometry, source signals and SNRs are the caller's, and so is the loop that replaces the rooms `simulate_rooms` marks invalid.
"""
import numpy as np

from .. import metrics
from .. import sigproc_utils as su
from .._engines import get_engine
from ..engine import DevBuf


def _engine():
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)      # these kernels do not depend on the batch geometry


def _node_slices(mics_per_node, n_mic):
    mpn = [int(m) for m in np.asarray(mics_per_node).reshape(-1)]
    if not mpn or min(mpn) < 1 or sum(mpn) != n_mic:
        raise ValueError(f'mics_per_node {mpn} does not add up to the {n_mic} channels of the signals')
    edges = np.concatenate([[0], np.cumsum(mpn)])
    return [slice(int(edges[i]), int(edges[i + 1])) for i in range(len(mpn))]


def snr_at_mics(s, n, mics_per_node, fs=16000, vad_s=None, vad_n=None, stop=None):
    """convolve_signals.py:170-213, batched: s, n (..., n_mic, L) -> (snrs (..., n_mic), nodes_snr (..., K), min_abs_delta (...)).
    snrs is the mean of metrics.fw_snr at every microphone (vad_s / vad_n shaped like s / n gate the band levels), nodes_snr its mean over
    the microphones of a node (mics_per_node may be ragged).  min_abs_delta is the reference's: its `delta_snrs` slices are filled with
    nodes_snr[i] - nodes_snr[i + 1] for i < K - 1 and nothing else (:208-211), so the smallest |difference| is taken over CONSECUTIVE
    nodes, not over all pairs.  One node has no difference: ValueError (the reference fails on its empty minimum).
    stop: None, a scalar, or an array broadcast over (..., n_mic)."""
    n_mic = int(s.shape[-2])
    nodes = _node_slices(mics_per_node, n_mic)
    if len(nodes) < 2:
        raise ValueError('snr_at_mics needs at least two nodes: the difference between nodes is undefined for one')
    snrs = np.asarray(metrics.fw_snr(s, n, fs, vad_tar=vad_s, vad_noi=vad_n, stop=stop)[1], np.float64)
    nodes_snr = np.stack([snrs[..., sl].mean(axis=-1) for sl in nodes], axis=-1)
    delta = nodes_snr[..., :-1] - nodes_snr[..., 1:]
    return snrs, nodes_snr, np.min(np.abs(delta), axis=-1)


def _dev(eng, a):
    """A float32 array on the device as it is, a NumPy array uploaded: -> something Engine methods answer with a DevBuf for."""
    if isinstance(a, DevBuf) or hasattr(a, 'data_ptr'):
        return a
    return eng.to_device(np.ascontiguousarray(a, dtype=np.float32), np.float32)[1]


def simulate_rooms(target_dry, noise_dry, room_dims, absorption, src_pos, mic_pos, mics_per_node, source_snr, snr_cnv_range, min_delta_snr,
                   fs=16000, max_order=20, rir_len=4096, target_vad=None, noise_vad=None, out_len=None):
    """simulate_room (convolve_signals.py:255-273) for R rooms at once, without files and without its redraw loop.
    target_dry, noise_dry (R, Ld); room_dims (R, 3), absorption (R,), src_pos (R, 2, 3) (target, noise), mic_pos (R, n_mic, 3).
      1. the target's VAD is vad_oracle_batch(target_dry) unless target_vad is given;
      2. the dry noise is scaled to source_snr (a scalar or one per room) with increase_to_snr(..., weight=True, vad_noi=noise_vad);
      3. Engine.ism_rir computes the RIRs, 4. Engine.rir_convolve the images of both sources (out_len samples, default Ld);
      5. image_vad = vad_oracle_batch(target images); 6. snr_at_mics(target images, noise images, vad_s=image_vad);
      7. valid[r] = all(lo < nodes_snr[r]) and all(nodes_snr[r] < hi) and min_delta_snr < snr_diff[r], (lo, hi) = snr_cnv_range.
    -> dict.  Device-resident (DevBuf), SOURCE-MAJOR so that each source's block is contiguous -- images[0] / images[1] are the target's /
    the noise's (R, n_mic, L) images and go to mix_rooms as they are: images (2, R, n_mic, L), rirs (2, R, n_mic, rir_len), image_vad
    (R, n_mic, L), noise_dry (R, Ld) the scaled dry noise.  NumPy: snr_images (R, n_mic), snr_nodes (R, K), snr_diff (R,), valid (R,) bool,
    noise_gain (R,).  The caller redraws the rooms that are not valid."""
    eng = _engine()
    target_dry, noise_in = _dev(eng, target_dry), _dev(eng, noise_dry)
    R, Ld = (int(v) for v in target_dry.shape)
    if tuple(int(v) for v in noise_in.shape) != (R, Ld):
        raise ValueError(f'target_dry and noise_dry must both be (R, Ld): {tuple(target_dry.shape)} and {tuple(noise_in.shape)}')
    room_dims = np.ascontiguousarray(room_dims, np.float32).reshape(R, 3)
    absorption = np.ascontiguousarray(absorption, np.float32).reshape(R)
    src_pos = np.ascontiguousarray(src_pos, np.float32)
    mic_pos = np.ascontiguousarray(mic_pos, np.float32)
    if src_pos.shape != (R, 2, 3) or mic_pos.ndim != 3 or mic_pos.shape[0] != R or mic_pos.shape[2] != 3:
        raise ValueError(f'src_pos must be ({R}, 2, 3) and mic_pos ({R}, n_mic, 3): {src_pos.shape} and {mic_pos.shape}')
    n_mic = int(mic_pos.shape[1])
    _node_slices(mics_per_node, n_mic)
    L = Ld if out_len is None else int(out_len)
    if target_vad is None:
        target_vad = su.vad_oracle_batch(target_dry)
    gain = np.broadcast_to(su.snr_gain(target_dry, noise_in, source_snr, vad_tar=target_vad, vad_noi=noise_vad, weight=True, fs=fs), (R,))
    # both dry sources in one source-major block: the target copied (gain 1 is exact), the noise scaled into its half
    dry = eng.empty((2, R, Ld), np.float32)
    eng.mix_scaled(None, target_dry, 1.0, n_out=dry[0])
    eng.mix_scaled(None, noise_in, gain, n_out=dry[1])
    two = lambda a: np.concatenate([a, a], axis=0)
    rirs = eng.ism_rir(two(room_dims), two(absorption), np.concatenate([src_pos[:, :1], src_pos[:, 1:]], axis=0), two(mic_pos),
                       max_order=max_order, fs=float(fs), rir_len=rir_len).reshape(2, R, n_mic, rir_len)
    images = eng.rir_convolve(dry.reshape(2 * R, Ld), rirs.reshape(2 * R, n_mic, rir_len), out_len=L).reshape(2, R, n_mic, L)
    image_vad = su.vad_oracle_batch(images[0])
    snr_images, snr_nodes, snr_diff = snr_at_mics(images[0], images[1], mics_per_node, fs, vad_s=image_vad)
    lo, hi = snr_cnv_range
    valid = np.all(lo < snr_nodes, axis=-1) & np.all(snr_nodes < hi, axis=-1) & (min_delta_snr < snr_diff)
    return dict(images=images, rirs=rirs, image_vad=image_vad, noise_dry=dry[1], snr_images=snr_images, snr_nodes=snr_nodes,
                snr_diff=snr_diff, valid=valid, noise_gain=np.array(gain, np.float64))


def reverb_at_mics(dry, rirs, reverb_start=20, fs=16000):
    """How reverberant the rooms of `simulate_rooms` came out: metrics.reverb_ratios (metrics.py:176-208) at every microphone.
    dry (R, Ld) with rirs (R, n_mic, rir_len), or source-major dry (S, R, Ld) with rirs (S, R, n_mic, rir_len) -- the `rirs` of
    simulate_rooms as they are; dry may also be a list of S (R, Ld) arrays, e.g. [target_dry, out['noise_dry']], which are copied into
    one source-major block.  NumPy arrays, device tensors or DevBufs.
    -> dict of NumPy arrays shaped like rirs without its last axis: drr, srr (dB) and split (the first tap of the tail, int32).
    One Engine.rir_split and one Engine.reverb_energies call for all sources; neither convolution is written to memory."""
    eng = _engine()
    if isinstance(dry, (list, tuple)):
        parts = [_dev(eng, d) for d in dry]
        R, Ld = (int(v) for v in parts[0].shape)
        block = eng.empty((len(parts), R, Ld), np.float32)
        for i, d in enumerate(parts):
            if tuple(int(v) for v in d.shape) != (R, Ld):
                raise ValueError(f'every dry source must be ({R}, {Ld}): source {i} is {tuple(d.shape)}')
            eng.mix_scaled(None, d, 1.0, n_out=block[i])              # gain 1 is exact: a copy
        dry = block
    dry, rirs = _dev(eng, dry), _dev(eng, rirs)
    lead = tuple(int(v) for v in dry.shape[:-1])
    if len(lead) not in (1, 2) or tuple(int(v) for v in rirs.shape[:len(lead)]) != lead or len(rirs.shape) != len(lead) + 2:
        raise ValueError(f'dry must be (R, Ld) with rirs (R, n_mic, rir_len), or (S, R, Ld) with (S, R, n_mic, rir_len): '
                         f'{tuple(dry.shape)} and {tuple(rirs.shape)}')
    n_sig = int(np.prod(lead, dtype=np.int64))
    n_mic, rir_len = int(rirs.shape[-2]), int(rirs.shape[-1])
    h = rirs.reshape(n_sig, n_mic, rir_len)
    split, e_h = eng.rir_split(h, int(1e-3 * reverb_start * fs))
    e_x = eng.reverb_energies(dry.reshape(n_sig, int(dry.shape[-1])), h, split).numpy()
    shape = lead + (n_mic,)
    return dict(drr=metrics._ratio_db(e_h.numpy()).reshape(shape), srr=metrics._ratio_db(e_x).reshape(shape), split=split.numpy().reshape(shape))


def mix_rooms(tar_img, noi_img, snr, mics_per_node, lengths=None):
    """PostGenerator.mix_sigs (post_generator.py:99-115) for R rooms: tar_img (R, n_mic, L), noi_img (R, n_mic, Ln <= L), one snr (dB) per
    room -> (y, s, n), each (R, K, M, L) on the device, ready for offline_tango_batched(y, s, n, lengths=lengths).  The noise is scaled by
    10 ** (-snr / 20) (a shorter one lands in a zero buffer, as the reference's) and y = s + n exactly (Engine.mix_scaled, one gain per
    room).  lengths (R,): y and n are zero at and beyond a room's length.  s is a view of tar_img, not a copy.  The path takes one M for
    every node: ragged mics_per_node raises ValueError."""
    mpn = [int(m) for m in np.asarray(mics_per_node).reshape(-1)]
    if len(set(mpn)) != 1:
        raise ValueError(f'mix_rooms needs the same number of microphones at every node, got mics_per_node = {mpn}')
    eng = _engine()
    tar_img, noi_img = _dev(eng, tar_img), _dev(eng, noi_img)
    R, n_mic, L = (int(v) for v in tar_img.shape)
    K, M = len(mpn), mpn[0]
    if K * M != n_mic or tuple(int(v) for v in noi_img.shape[:2]) != (R, n_mic):
        raise ValueError(f'mics_per_node {mpn} / noi_img {tuple(noi_img.shape)} do not fit tar_img {tuple(tar_img.shape)}')
    try:
        gain = 10 ** (-np.broadcast_to(np.asarray(snr, np.float64), (R,)) / 20)
    except ValueError:
        raise ValueError(f'snr of shape {np.shape(snr)} is not one value per room ({R})') from None
    stop = None
    if lengths is not None:
        try:
            stop = np.broadcast_to(np.asarray(lengths), (R,))[:, None]
        except ValueError:
            raise ValueError(f'lengths of shape {np.shape(lengths)} is not one value per room ({R})') from None
    n, y = eng.mix_scaled(tar_img, noi_img, gain, group=n_mic, stop=stop)
    return y.reshape(R, K, M, L), tar_img.reshape(R, K, M, L), n.reshape(R, K, M, L)
