"""Meeting rooms of S simultaneous talkers, where talker i is the target of node i (the reference's second generator,
dataset_generation/gen_meetit/convolve_signals.py), for R rooms at once and without files, geometry draws or the redraw loop.

    get_value_range     :43-56      the range of values a RIR index falls into
    sir_at_nodes        :81-91, 140-148    BSS-eval SIR of every node's own talker against the sum of the others
    sir_valid           :94-111, 150-152, 271-289    check_sir_validity over a sequence of rooms, with the history it builds
    simulate_meetings   :114-163    RIRs, images and SIRs of R rooms
    meeting_rooms                   (y, s, n) per node for offline_tango_batched: a different target per node
    meeting_masks       :166-188    get_masks: the mix spectrum and every talker's mask at every channel

Images are SOURCE-MAJOR on the device, (S, R, n_mic, L), so that each talker's block is contiguous (the layout of simulate_rooms).  The
signals stay on the device (DevBuf); the figures (SIRs, verdicts) are NumPy.  2 <= S <= 8.
"""
import numpy as np

from .. import metrics
from .._engines import get_engine
from .rooms import _dev, _engine, _node_slices


def get_value_range(i_rir, n_rirs, vmin=0, vmax=20, n_bins=5):
    """convolve_signals.py:43-56: [vmin, vmax] cut into n_bins equal ranges -> the (lo, hi) of the range RIR index i_rir of n_rirs falls into
    (the bin index is the reference's float floor division i_rir // (n_rirs / n_bins))."""
    i_bin = i_rir // (n_rirs / n_bins)
    span = vmax - vmin
    return np.array([vmin + i_bin * span / n_bins, vmin + (i_bin + 1) * span / n_bins])


def _node_targets(mics_per_node, n_mic):
    """-> (node slices, target (n_mic,) int32: channel c listens to the talker with its node's index)."""
    nodes = _node_slices(mics_per_node, n_mic)
    target = np.concatenate([np.full(sl.stop - sl.start, k, np.int32) for k, sl in enumerate(nodes)])
    return nodes, target


def _room_stops(lengths, R, name='lengths'):
    """None, or one length per room -> None or (R, 1), which broadcasts over the channels of a room."""
    if lengths is None:
        return None
    try:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(lengths), (R,)))[:, None]
    except ValueError:
        raise ValueError(f'{name} of shape {np.shape(lengths)} is not one value per room ({R})') from None


def _images(eng, images):
    images = _dev(eng, images)
    shape = tuple(int(v) for v in images.shape)
    if len(shape) != 4:
        raise ValueError(f'images must be (S, R, n_mic, L), source-major: {shape}')
    return images, shape


def sir_at_nodes(images, mics_per_node, stop=None):
    """images (S, R, n_mic, L) -> SIRs (R, S) in dB: for node i and each of its microphones, SIR[0] of bss_eval_sources(refs = (s_i, n_i),
    ests = (m, m), compute_permutation=False) with s_i the image of talker i, n_i the sum of all other images and m = s_i + n_i, averaged
    over the node's microphones (sir_at_node, convolve_signals.py:81-91, called as at :140-148).  s_i and n_i are Engine.source_mix's
    (n_i summed in ascending talker order); mics_per_node may be ragged but names exactly S nodes.  stop: None, or one length per room."""
    eng = _engine()
    images, (S, R, n_mic, L) = _images(eng, images)
    nodes, target = _node_targets(mics_per_node, n_mic)
    if len(nodes) != S:
        raise ValueError(f'{S} sources need {S} nodes (node i listens to source i): mics_per_node names {len(nodes)}')
    stops = _room_stops(stop, R, 'stop')
    _, s, n = eng.source_mix(images, target, stop=stops, want_y=False)
    s, n = s.numpy(), n.numpy()
    refs = np.stack([s, n], axis=-2)                                         # (R, n_mic, 2, L)
    m = s + n
    ests = np.stack([m, m], axis=-2)
    span = None if stops is None else np.ascontiguousarray(np.broadcast_to(stops, (R, n_mic)))
    sir = metrics.bss_eval_sources(refs, ests, compute_permutation=False, stop=span)[1][..., 0]          # (R, n_mic)
    return np.stack([sir[:, sl].mean(axis=-1) for sl in nodes], axis=-1)


def sir_classes(n_rirs_per_proc, n_classes=4):
    """convolve_signals.py:150-152 -> (starts, stops, level): classes [2 + 3 k, 2 + 3 (k + 1)] dB, each to hold ceil(n_rirs_per_proc /
    n_classes) rooms."""
    starts = [2 + 3 * k for k in range(n_classes)]
    return starts, [b + 3 for b in starts], float(np.ceil(n_rirs_per_proc / n_classes))


def _sir_verdict(current, past, classes, delta_sir):
    """check_sir_validity (convolve_signals.py:94-111) as written.  Its quirks, kept: the differences are taken against ROLLED copies of
    the SIRs (so every ordered pair is tested, through len(past) - 1 shifts) and only an excess counts (no absolute value); only the FIRST
    source's SIR is classed and only the first source's history is binned; every comparison is strict, so a class accepts one room more
    than its level and an SIR on the outer edges 2 dB / 14 dB passes the range test.  (An SIR of exactly the lowest edge then finds no class
    start below it: IndexError, as in the reference.)  np.histogram is what plt.hist calls."""
    starts, stops, level = classes
    for shift in range(1, len(past)):
        if np.any((current - np.roll(current, shift)) > delta_sir):
            return False
    if current[0] < starts[0] or current[0] > stops[-1]:
        return False
    i_class = np.where(current[0] > starts)[0][-1]
    filled = np.histogram(past[0], bins=len(starts), range=(starts[0], stops[-1]))[0]
    return not filled[i_class] > level


def sir_valid(sirs, n_rirs_per_proc, past=None, delta_sir=2):
    """sirs (R, S): the SIRs of R rooms in the order they were drawn -> (valid (R,) bool, past).  Room r is judged by check_sir_validity
    (`_sir_verdict`) with the classes of `sir_classes(n_rirs_per_proc)` against the history `past`, a list of S lists (None: empty); an
    accepted room's SIRs join the history before the next room is judged, as in the loop at convolve_signals.py:271-289.  `past` is
    returned extended (the caller's list is not modified)."""
    sirs = np.asarray(sirs, np.float64)
    if sirs.ndim != 2:
        raise ValueError(f'sirs must be (R, S): {sirs.shape}')
    R, S = sirs.shape
    past = [[] for _ in range(S)] if past is None else [list(p) for p in past]
    if len(past) != S:
        raise ValueError(f'past must hold one list per source ({S}): {len(past)}')
    classes = sir_classes(n_rirs_per_proc)
    valid = np.zeros(R, bool)
    for r in range(R):
        valid[r] = _sir_verdict(sirs[r], past, classes, delta_sir)
        if valid[r]:
            for k in range(S):
                past[k].append(float(sirs[r, k]))
    return valid, past


def simulate_meetings(sources_dry, room_dims, absorption, src_pos, mic_pos, mics_per_node, fs=16000, max_order=20, rir_len=4096,
                      out_len=None, lengths=None):
    """simulate_room (convolve_signals.py:114-163) for R rooms at once, without files, draws or its redraw rule.
    sources_dry (R, S, Ld); room_dims (R, 3), absorption (R,), src_pos (R, S, 3), mic_pos (R, n_mic, 3); S must equal the number of nodes
    (the reference indexes nodes by source).  One Engine.ism_rir call computes the RIRs of all S sources and one Engine.rir_convolve call
    their images of out_len samples (default Ld): the reference's pad-or-truncate to len_max (:157-161), zeros beyond Ld + rir_len - 1.
    lengths (R,): the SIRs are scored below each room's length.
    -> dict.  On the device, source-major: images (S, R, n_mic, L), rirs (S, R, n_mic, rir_len).  NumPy: sirs (R, S) (`sir_at_nodes`).
    Nothing is drawn or redrawn: `sir_valid` gives the verdicts, the caller replaces the rooms."""
    eng = _engine()
    mic_pos = np.ascontiguousarray(mic_pos, np.float32)
    src_pos = np.ascontiguousarray(src_pos, np.float32)
    shape = tuple(int(v) for v in sources_dry.shape)
    if len(shape) != 3:
        raise ValueError(f'sources_dry must be (R, S, Ld): {shape}')
    R, S, Ld = shape
    if src_pos.shape != (R, S, 3) or mic_pos.ndim != 3 or mic_pos.shape[0] != R or mic_pos.shape[2] != 3:
        raise ValueError(f'src_pos must be ({R}, {S}, 3) and mic_pos ({R}, n_mic, 3): {src_pos.shape} and {mic_pos.shape}')
    n_mic = int(mic_pos.shape[1])
    n_nodes = len(_node_slices(mics_per_node, n_mic))
    if n_nodes != S:
        raise ValueError(f'{S} sources need {S} nodes (node i listens to source i): mics_per_node names {n_nodes}')
    room_dims = np.ascontiguousarray(room_dims, np.float32).reshape(R, 3)
    absorption = np.ascontiguousarray(absorption, np.float32).reshape(R)
    L = Ld if out_len is None else int(out_len)
    # the dry sources source-major: a host array is transposed before its upload, a device array copied block by block (gain 1 is exact)
    if isinstance(sources_dry, np.ndarray) or not (hasattr(sources_dry, 'ptr') or hasattr(sources_dry, 'data_ptr')):
        dry = _dev(eng, np.ascontiguousarray(np.swapaxes(np.asarray(sources_dry, np.float32), 0, 1)))
    else:
        src = _dev(eng, sources_dry)
        if not hasattr(src, 'part'):
            raise ValueError('device-resident sources_dry must be a DevBuf (or pass a NumPy array)')
        dry = eng.empty((S, R, Ld), np.float32)
        for r in range(R):
            for i in range(S):
                eng.mix_scaled(None, src[r][i].reshape(1, Ld), 1.0, n_out=dry[i][r].reshape(1, Ld))
    # every (source, room) as a room of one source, so that the RIRs come out source-major from one call
    tile = lambda a: np.concatenate([a] * S, axis=0)
    rirs = eng.ism_rir(tile(room_dims), tile(absorption), np.ascontiguousarray(np.swapaxes(src_pos, 0, 1)).reshape(S * R, 1, 3), tile(mic_pos),
                       max_order=max_order, fs=float(fs), rir_len=rir_len).reshape(S, R, n_mic, rir_len)
    images = eng.rir_convolve(dry.reshape(S * R, Ld), rirs.reshape(S * R, n_mic, rir_len), out_len=L).reshape(S, R, n_mic, L)
    return dict(images=images, rirs=rirs, sirs=sir_at_nodes(images, mics_per_node, stop=lengths))


def meeting_rooms(images, mics_per_node, lengths=None):
    """images (S, R, n_mic, L) -> (y, s, n), each (R, K, M, L) on the device, ready for offline_tango_batched(y, s, n, lengths=lengths):
    at node k, s is talker k's image, n the sum of the others and y the mix of all (Engine.source_mix; for S >= 3 y is the left-to-right
    sum of the images, which need not be s + n to the last bit).  lengths (R,): zeros at and beyond a room's length.  The path takes one
    M for every node: ragged mics_per_node raises ValueError, as mix_rooms does; K must be S."""
    mpn = [int(m) for m in np.asarray(mics_per_node).reshape(-1)]
    if len(set(mpn)) != 1:
        raise ValueError(f'meeting_rooms needs the same number of microphones at every node, got mics_per_node = {mpn}')
    eng = _engine()
    images, (S, R, n_mic, L) = _images(eng, images)
    nodes, target = _node_targets(mpn, n_mic)
    K, M = len(mpn), mpn[0]
    if K != S:
        raise ValueError(f'{S} sources need {S} nodes (node i listens to source i): mics_per_node names {K}')
    y, s, n = eng.source_mix(images, target, stop=_room_stops(lengths, R))
    return y.reshape(R, K, M, L), s.reshape(R, K, M, L), n.reshape(R, K, M, L)


def meeting_masks(images, mics_per_node=None, lengths=None, type='irm1', n_fft=512):
    """get_masks (convolve_signals.py:166-188) for R rooms: images (S, R, n_mic, L) -> (stfts (R, n_mic, T, F) complex64, masks
    (S, R, n_mic, T, F)), on the device: the spectrum of every channel's mix and, at every channel, the `type` mask of every talker against
    the sum of the others (Engine.source_masks: one transform pass, the sums taken on the spectra).  The reference's walk over the nodes
    visits every channel once, in order: mics_per_node is only checked against n_mic.  lengths (R,): per-room clip lengths
    (Engine.set_lengths)."""
    images, (S, R, n_mic, L) = _images(_engine(), images)
    if mics_per_node is not None:
        _node_slices(mics_per_node, n_mic)
    eng = get_engine(rooms=R, nodes=1, mics=n_mic, length=L, n_fft=n_fft, mask=type)
    try:                                                                     # (a cached engine: the lengths do not outlive the call)
        if lengths is not None:
            eng.set_lengths(lengths)
        masks, mix = eng.source_masks(images.reshape(S, R * n_mic, L))
    finally:
        if lengths is not None:
            eng.set_lengths(None)
    return mix.reshape(R, n_mic, eng.T, eng.F), masks.reshape(S, R, n_mic, eng.T, eng.F)
