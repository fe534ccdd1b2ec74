"""Checks of the training bank filled from rooms, shared by test_bank_cpu.py (what needs no library: refusals of from_rooms, the file
names, get_input_lists, get_dset), test_bank_emulated.py (the kernel and the package under hipemu) and test_gpu_bank.py (the MI355X).

Kernel checks take a bound library and a torch device and go through the C ABI (disco_bank_fill); the checks of the Python surface
(SpectraBank.from_rooms, dataset_utils.post, dnn.utils.get_input_lists) take the device only and use the package's cached engines: under
the emulator the caller has put the emulated library in disco_amd._lib._lib.

Bound of the magnitudes, 2 ** -22 relative to the float64 magnitude: sqrtf(fmaf(x, x, y * y)) has one rounding in y * y and one in the fma,
each at most 2 ** -24 of the sum and halved by the root, and the root's own rounding of 2 ** -24: under 3 ulp.  Inputs are drawn with
1e-6 <= |a| <= 1e6, so nothing underflows.  Where the other side is np.abs of the same complex64 value (itself within an ulp), the same
bound is used.  Masks, zeros and untouched elements are compared bit for bit."""
import os

import numpy as np
import torch

from disco_amd import _engines
from disco_amd.dnn import data as D

E_ARG = -1
SENTINEL = -7.0
REL = 2.0 ** -22
MASK_SPECIALS = np.array([np.nan, np.inf, -np.inf, 1e-42, -0.0, 0.0], np.float32)      # NaN, infinities, a denormal, both zeros


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sync(dev):
    if str(dev).startswith('cuda'):
        torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _complex(rng, shape):
    """complex64 with 1e-6 <= |a| <= 1e6, log-uniform in magnitude"""
    mag = 10.0 ** rng.uniform(-6, 6, shape)
    ph = rng.uniform(0, 2 * np.pi, shape)
    return np.clip(mag, 1.0001e-6, 0.9999e6) * np.exp(1j * ph)


# ---- the kernel through the C ABI ------------------------------------------------------------------------------------------------------------

def make_case(R=3, K=2, T=9, F=17, M=3, mic=1, z=(True, True), frames=(9, 4, 6), skip=2, N=5, Tb=8, seg0=1, seed=0, specials=True):
    rng = np.random.default_rng(seed)
    c = dict(R=R, K=K, T=T, F=F, M=M, mic=mic, skip=skip, N=N, Tb=Tb, seg0=seg0)
    c['X'] = _complex(rng, (R, K, T, F, M)).astype(np.complex64)
    c['z'] = [_complex(rng, (R, K, T, F)).astype(np.complex64) if present else None for present in z]
    mask = rng.random((R, K, T, F)).astype(np.float32)
    if specials:
        flat = mask.reshape(-1)
        flat[rng.choice(flat.size, 4 * MASK_SPECIALS.size, replace=False)] = np.tile(MASK_SPECIALS, 4)
        if F > MASK_SPECIALS.size and skip < T:
            mask[0, K - 1, skip, 1:1 + MASK_SPECIALS.size] = MASK_SPECIALS          # one of each in a frame every case with frames[0] > skip keeps
        c['X'][0, 0, skip, 0, mic] = np.nan                                         # NaN passes through the magnitude
        if c['z'][0] is not None:
            c['z'][0][0, K - 1, skip, F - 1] = complex(np.inf, 1.0)
    c['mask'] = mask
    c['frames'] = None if frames is None else np.asarray(frames, np.int32)
    return c


def restate(c):
    """The NumPy restatement: -> (want (S, N, Tb, F) float64 with the sentinel wherever nothing is written, is_mag (S,) rows that hold
    magnitudes).  Mask rows hold the source's float32 values exactly (float64 holds every float32)."""
    R, K, T, F, Tb, skip = c['R'], c['K'], c['T'], c['F'], c['Tb'], c['skip']
    zs = [z for z in c['z'] if z is not None]
    S = K * (2 + len(zs))
    want = np.full((S, c['N'], Tb, F), SENTINEL, np.float64)
    with np.errstate(all='ignore'):
        src = [np.abs(c['X'][..., c['mic']].astype(np.complex128))] + [np.abs(z.astype(np.complex128)) for z in zs] + [c['mask'].astype(np.float64)]
    for r in range(R):
        n_src = T if c['frames'] is None else min(int(c['frames'][r]), T)
        nf = min(max(n_src - skip, 0), Tb)
        for i, a in enumerate(src):
            for k in range(K):
                want[i * K + k, c['seg0'] + r, :nf] = a[r, k, skip:skip + nf]
                want[i * K + k, c['seg0'] + r, nf:] = 0.0
    is_mag = np.repeat(np.arange(2 + len(zs)) <= len(zs), K)
    return want, is_mag


def call_fill(lib, dev, c, **override):
    """-> (rc, bank as NumPy).  override: arguments replaced after marshalling (the refusals)."""
    zs = [z for z in c['z'] if z is not None]
    S = c['K'] * (2 + len(zs))
    keep = [_dev(c['X'], dev), [None if z is None else _dev(z, dev) for z in c['z']], _dev(c['mask'], dev),
            None if c['frames'] is None else _dev(c['frames'], dev)]
    bank = torch.full((S, c['N'], c['Tb'], c['F']), SENTINEL, dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    a = dict(X=p(keep[0]), z0=p(keep[1][0]), z1=p(keep[1][1]), mask=p(keep[2]), frames=p(keep[3]), R=c['R'], K=c['K'], M=c['M'], T=c['T'], F=c['F'],
             mic=c['mic'], n_zsig=len(zs), skip=c['skip'], bank=bank.data_ptr(), N=c['N'], Tb=c['Tb'], seg0=c['seg0'])
    a.update(override)
    rc = lib.disco_bank_fill(None, a['X'], a['z0'], a['z1'], a['mask'], a['frames'], a['R'], a['K'], a['M'], a['T'], a['F'], a['mic'], a['n_zsig'],
                             a['skip'], a['bank'], a['N'], a['Tb'], a['seg0'], None)
    _sync(dev)
    return rc, bank.cpu().numpy()


def compare(got, want, is_mag, what=''):
    """Magnitude rows within REL of the float64 magnitude (NaN where it is NaN, inf where it is inf); everything else -- mask rows, the zeros
    beyond a room's frames, the elements nothing writes -- bit for bit."""
    exact = np.ones(want.shape, bool)
    mag = (want != SENTINEL) & is_mag[:, None, None, None]
    exact[mag] = False
    assert np.array_equal(_bits(got[exact]), _bits(want[exact].astype(np.float32))), (what, 'masks / zeros / untouched elements differ in their bits')
    g, w = got[mag].astype(np.float64), want[mag]
    fin = np.isfinite(w)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (what, 'NaN / inf')
    err = np.abs(g[fin] - w[fin])
    assert bool((err <= REL * w[fin]).all()), (what, float((err / np.maximum(w[fin], 1e-300)).max()) / REL)
    zeros = (want == 0) & mag
    assert not _bits(got[zeros]).any(), (what, 'a zero beyond the frames is not +0.0')
    return float((err / np.maximum(w[fin], 1e-300)).max()) if fin.any() else 0.0


def _features(lib, dev, c, Z):
    """|X[..., mic]| and |Z| as disco_crnn_features gives them with lo = 0, hi = inf (crnn_features_hip(X, Z, mic, (0, 0), lo=0.0, hi=inf)):
    -> (R, K, T, F) of the mixture, (R, K, T, F) of Z (node j's plane is channel 1 + (j, or j - 1 past k) of any other node k)."""
    R, K, T, F, M = (c[k] for k in 'RKTFM')
    Xd, Zd = _dev(c['X'], dev), _dev(Z, dev)
    out = torch.empty((R * K, K, T, F), dtype=torch.float32, device=dev)
    assert lib.disco_crnn_features(None, Xd.data_ptr(), Zd.data_ptr(), R, K, M, T, F, c['mic'], 0, 0, 0.0, float('inf'), out.data_ptr(), None) == 0
    _sync(dev)
    o = out.cpu().numpy().reshape(R, K, K, T, F)
    zmag = np.stack([o[:, (j + 1) % K, 1 + (j if j < (j + 1) % K else j - 1)] for j in range(K)], axis=1)
    return o[:, :, 0], zmag


def check_main_case(lib, dev):
    c = make_case()
    R, K, skip, seg0 = c['R'], c['K'], c['skip'], c['seg0']
    rc, got = call_fill(lib, dev, c)
    assert rc == 0, rc
    want, is_mag = restate(c)
    assert (got[:, [0, 4]] == SENTINEL).all(), 'segments 0 and 4 keep the sentinel'
    mask_rows = got[3 * K:, seg0:seg0 + R]
    assert np.isnan(mask_rows).any() and np.isinf(mask_rows).any() and (mask_rows == np.float32(1e-42)).any() and np.signbit(mask_rows[mask_rows == 0]).any()
    assert np.isnan(got[0, seg0, 0, 0]) and np.isinf(got[K + K - 1, seg0, 0, c['F'] - 1]), 'NaN / inf pass through the magnitude'
    worst = compare(got, want, is_mag, 'main case')
    # bit-equal to the inference features at the same elements
    xmag, z0mag = _features(lib, dev, c, c['z'][0])
    _, z1mag = _features(lib, dev, c, c['z'][1])
    for i, a in enumerate((xmag, z0mag, z1mag)):
        for r in range(R):
            nf = min(max(min(int(c['frames'][r]), c['T']) - skip, 0), c['Tb'])
            assert nf < c['Tb'] or r == 0
            for k in range(K):
                assert np.array_equal(_bits(got[i * K + k, seg0 + r, :nf]), _bits(a[r, k, skip:skip + nf])), (i, r, k)
                assert not _bits(got[i * K + k, seg0 + r, nf:]).any(), 'exact zeros at tb >= min(frames[r], T) - skip'
    return worst


VARIANTS = {
    'no_z': dict(z=(False, False)),
    'z0_only': dict(z=(True, False)),
    'z1_only': dict(z=(False, True)),
    'one_mic': dict(M=1, mic=0),
    'frames_null': dict(frames=None),
    'skip_0': dict(skip=0, Tb=9),
    'room_all_skipped': dict(frames=(9, 2, 1), skip=2),
    'frames_above_T': dict(frames=(9, 14, 6)),
    'bank_shorter': dict(Tb=4, frames=(9, 9, 5)),
    'F257': dict(R=1, T=3, F=257, frames=(3,), skip=1, N=1, Tb=3, seg0=0),
    # a plane of more than 256 chunks of 1024 elements: the workgroups of a plane take a second pass
    'second_pass_of_a_plane': dict(R=1, K=1, T=1030, F=257, M=1, mic=0, z=(False, False), frames=(1027,), skip=1, N=1, Tb=1027, seg0=0, specials=False),
}


def check_variant(lib, dev, name):
    c = make_case(seed=1 + sorted(VARIANTS).index(name), **VARIANTS[name])
    rc, got = call_fill(lib, dev, c)
    assert rc == 0, (name, rc)
    want, is_mag = restate(c)
    if name == 'room_all_skipped':
        assert not _bits(got[:, c['seg0'] + 1:c['seg0'] + 3]).any(), 'skip >= frames[r]: all zeros'
    return compare(got, want, is_mag, name)


def check_refusals(lib, dev):
    c = make_case()
    bad = dict(no_X=dict(X=None), no_mask=dict(mask=None), no_bank=dict(bank=None), mic_low=dict(mic=-1), mic_high=dict(mic=c['M']),
               skip_negative=dict(skip=-1), Tb_zero=dict(Tb=0), seg0_negative=dict(seg0=-1), past_the_bank=dict(seg0=c['N'] - c['R'] + 1),
               n_zsig_low=dict(n_zsig=1), n_zsig_high=dict(n_zsig=3), z_missing=dict(z1=None), z0_missing=dict(z0=None, n_zsig=2))
    for name, override in bad.items():
        rc, got = call_fill(lib, dev, c, **override)
        assert rc == E_ARG, (name, rc)
        assert (got == SENTINEL).all(), (name, 'a refused call wrote to the bank')
    return len(bad)


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------------

N_FFT, HOP, SKIP, WIN = 512, 256, 3, 21
R_, K_, M_ = 3, 2, 2
FRAMES = np.array([24, 27, 30])
LENGTHS = (FRAMES - 1) * HOP + 19
L_ = int(LENGTHS.max())
REF = 2                                     # reference channel, counted from 1: microphone 1 of every node
SNR = np.array([1.5, 3.0, 5.5])
_shared = {}


def shared(key, make):
    """One value per key for the whole run (references are computed once and left unchanged); dropped when the library under test changes."""
    from disco_amd import _lib
    lib = _lib.load()                       # the emulated library where a test has bound it, else the gfx950 one
    if _shared.get('lib') is not lib:
        _shared.clear()
        _shared['lib'] = lib
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def images():
    rng = np.random.default_rng(42)
    tar = (0.1 * rng.standard_normal((R_, K_ * M_, L_))).astype(np.float32)
    noi = (0.1 * rng.standard_normal((R_, K_ * M_, L_))).astype(np.float32)
    return tar, noi


def rooms_dev():
    """y, s, n (R, K, M, L) DevBufs: what mix_rooms returns for the images"""
    from disco_amd.dataset_utils import mix_rooms
    return shared('rooms_dev', lambda: mix_rooms(*images(), SNR, (M_,) * K_, lengths=LENGTHS))


def rooms_host():
    return shared('rooms_host', lambda: tuple(a.numpy() for a in rooms_dev()))


def _engine(ref_mic, R=R_):
    return _engines.get_engine(rooms=R, nodes=K_, mics=M_, length=L_, n_fft=N_FFT, mask='irm1', pad_mode='reflect', ref_mic=ref_mic, mu=1.0,
                               staged_step2=True)


def step1():
    """The path's own outputs: offline_tango_batched(steps=1) and Engine.stft of the nodes' channels, as host arrays"""
    from disco_amd.speech_enhancement.tango import offline_tango_batched

    def make():
        y, s, n = rooms_host()
        out = offline_tango_batched(y, s, n, vads='irm1', ref_mic=REF - 1, steps=1, lengths=LENGTHS)
        eng = _engine(REF - 1)
        try:
            eng.set_lengths(LENGTHS)
            out['X'] = eng.stft(y.reshape(R_ * K_, M_, L_)).numpy().reshape(R_, K_, eng.T, eng.F, M_)
        finally:
            eng.set_lengths(None)
        return out
    return shared('step1', make)


def bank_of(z_sigs, **kw):
    key = ('bank', str(z_sigs), tuple(sorted(kw.items())))
    return shared(key, lambda: D.SpectraBank.from_rooms(*rooms_host(), lengths=LENGTHS, z_sigs=z_sigs, ref_channel=REF, skip_frames=SKIP,
                                                        n_fft=N_FFT, win_len=WIN, **kw))


def expected_by_hand(z_sigs):
    """(S, N, F, T) in the reference's orientation from the path's own outputs: float64 magnitudes of the complex64 values, the masks as they
    are, zeros beyond n_frames."""
    o = step1()
    names = [] if z_sigs is None else ([z_sigs] if isinstance(z_sigs, str) else z_sigs)
    src = [np.abs(o['X'][..., REF - 1].astype(np.complex128))] + [np.abs(o[D.Z_OUTPUTS[nm]].astype(np.complex128)) for nm in names] + \
        [o['masks_z'].astype(np.float64)]
    n_frames = FRAMES - SKIP
    want = np.zeros((K_ * len(src), R_, 257, int(n_frames.max())))
    for i, a in enumerate(src):
        for r in range(R_):
            for k in range(K_):
                want[i * K_ + k, r, :, :n_frames[r]] = a[r, k, SKIP:FRAMES[r]].T
    return want, np.repeat(np.arange(len(src)) < len(src) - 1, K_)


def _same_banks(got, want, is_mag, what):
    """got (S, N, T, F) float32 against want (S, N, T, F): mask rows bit-equal, magnitude rows within REL, exact zeros where want is zero."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got[~is_mag]), _bits(want[~is_mag].astype(np.float32))), (what, 'mask rows')
    g, w = got[is_mag].astype(np.float64), want[is_mag].astype(np.float64)
    assert np.isfinite(w).all() and bool((np.abs(g - w) <= REL * w).all()), (what, float((np.abs(g - w) / np.maximum(w, 1e-300)).max()) / REL)
    return float((np.abs(g - w) / np.maximum(w, 1e-300)).max()) / REL


def check_from_rooms(z_sigs):
    bank = bank_of(z_sigs)
    want, is_mag = expected_by_hand(z_sigs)
    assert np.array_equal(bank.n_frames, FRAMES - SKIP) and bank.n_nodes == K_ and (bank.S, bank.N, bank.T, bank.F) == (want.shape[0], R_, 27, 257)
    assert bank.data.dtype == torch.float32 and bank.data.is_contiguous()
    got = bank.data.cpu().numpy()
    for r in range(R_):
        assert not _bits(got[:, r, bank.n_frames[r]:]).any(), 'exact zeros beyond n_frames'
        assert got[:, r, :bank.n_frames[r]].any()
    return _same_banks(got, want.transpose(0, 1, 3, 2), is_mag, f'from_rooms {z_sigs}')


def check_rooms_per_call():
    whole = bank_of('zs_hat', rooms_per_call=2).data.cpu().numpy()
    y, s, n = rooms_host()
    for r0, r1 in ((0, 2), (2, 3)):
        part = D.SpectraBank.from_rooms(y[r0:r1], s[r0:r1], n[r0:r1], lengths=LENGTHS[r0:r1], z_sigs='zs_hat', ref_channel=REF, skip_frames=SKIP,
                                        n_fft=N_FFT, win_len=WIN)
        assert np.array_equal(part.n_frames, (FRAMES - SKIP)[r0:r1])
        p = part.data.cpu().numpy()
        assert np.array_equal(_bits(whole[:, r0:r1, :part.T]), _bits(p)) and not _bits(whole[:, r0:r1, part.T:]).any(), (r0, r1)
    return True


def check_device_inputs(dev):
    """The DevBufs of mix_rooms, device tensors of the same values and host copies give the same bank bit for bit (in pieces of two rooms, so
    that every container is also cut)."""
    host = bank_of('zs_hat', rooms_per_call=2).data.cpu().numpy()
    kw = dict(lengths=LENGTHS, z_sigs='zs_hat', ref_channel=REF, skip_frames=SKIP, n_fft=N_FFT, win_len=WIN, rooms_per_call=2)
    from_bufs = D.SpectraBank.from_rooms(*rooms_dev(), **kw)
    assert np.array_equal(_bits(from_bufs.data.cpu().numpy()), _bits(host)), 'DevBuf inputs'
    from_tensors = D.SpectraBank.from_rooms(*(_dev(a, dev) for a in rooms_host()), **kw)
    assert np.array_equal(_bits(from_tensors.data.cpu().numpy()), _bits(host)), 'tensor inputs'
    assert str(from_bufs.data.device).split(':')[0] == str(dev).split(':')[0]
    return True


def check_bad_inputs():
    """ValueError before any launch: with no library and no GPU these must still be ValueError, and they are checked there (test_bank_cpu.py)."""
    import pytest
    rng = np.random.default_rng(0)
    y = rng.standard_normal((2, 2, 2, 24 * HOP)).astype(np.float32)                 # 25 frames
    kw = dict(skip_frames=SKIP, n_fft=N_FFT, win_len=WIN)
    with pytest.raises(ValueError, match='room 1'):
        D.SpectraBank.from_rooms(y, y, y, lengths=[24 * HOP, 22 * HOP + 255], **kw)                # 23 frames - 3 < 21
    with pytest.raises(ValueError, match='room 0'):
        D.SpectraBank.from_rooms(y, y, y, skip_frames=5, n_fft=N_FFT, win_len=WIN)
    for bad in ('irm', 'snr1', 'crnn', 'ivad', None):
        with pytest.raises(ValueError, match='mask type'):
            D.SpectraBank.from_rooms(y, y, y, mask_type=bad, **kw)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match='ref_channel'):
            D.SpectraBank.from_rooms(y, y, y, ref_channel=bad, **kw)
    with pytest.raises(ValueError, match='z_sigs'):
        D.SpectraBank.from_rooms(y, y, y, z_sigs='z_hat', **kw)
    with pytest.raises(ValueError, match='lengths'):
        D.SpectraBank.from_rooms(y, y, y, lengths=[24 * HOP + 1, 100], **kw)
    with pytest.raises(ValueError):
        D.SpectraBank.from_rooms(y, y, y[:1], **kw)
    return True


def check_batches_and_a_training_step():
    from disco_amd.dnn import train as TR
    bank = D.SpectraBank.from_rooms(*rooms_host(), lengths=LENGTHS, z_sigs=['zs_hat', 'zn_hat'], ref_channel=REF, skip_frames=SKIP, n_fft=N_FFT,
                                    win_len=WIN, stack_axis=2)
    assert bank.n_ch == 1 + (K_ - 1) * 2 and len(bank) == 3                       # 21, 24 and 27 frames: one window of 21 at hop 8 each
    got = list(D.batches(bank, 8, np.random.default_rng(5)))
    rng = np.random.default_rng(5)                                               # the same draws, by hand
    tab = bank.draw_batch(rng.permutation(len(bank)), rng)
    assert len(got) == 1
    x, y = got[0]
    B, C = tab.shape[0], bank.n_ch
    assert tuple(x.shape) == (B, C, WIN, 257) and tuple(y.shape) == (B, WIN, 257) and x.device == bank.data.device
    data = bank.data.cpu().numpy()
    for b, row in enumerate(tab):
        k, m = row[0], row[1]
        for c in range(C):
            assert np.array_equal(_bits(x[b, c].cpu().numpy()), _bits(data[row[2 + c], k, m:m + WIN])), (b, c)
        assert np.array_equal(_bits(y[b].cpu().numpy()), _bits(data[row[-1], k, m:m + WIN])), b
    torch.manual_seed(3)
    model, opt = TR.load_architecture(C)
    model.to(bank.data.device)
    loss = TR.train_one_batch(model, x, y, opt, 'all')
    assert np.isfinite(loss), loss
    return float(loss)


RIR_IDS = (11, 12, 13)


def post():
    from disco_amd.dataset_utils import post_process_rooms
    return shared('post', lambda: post_process_rooms(*images(), SNR, (M_,) * K_, lengths=LENGTHS, mask_type='irm1', n_fft=N_FFT))


def check_post_channel(k=1, m=0):
    """post_process_rooms at a channel that is no reference microphone: mask and mixture spectrum are Engine.tf_mask and Engine.stft of that
    channel bit for bit; the mix is mix_rooms'."""
    p = post()
    y, s, n = rooms_host()
    assert np.array_equal(_bits(p['y'].numpy()), _bits(y.reshape(R_, K_ * M_, L_))) and np.array_equal(_bits(p['n'].numpy()), _bits(n.reshape(R_, -1, L_)))
    assert np.array_equal(p['frames'], FRAMES) and np.array_equal(p['lengths'], LENGTHS) and m != REF - 1
    eng = _engine(0)
    try:
        eng.set_lengths(LENGTHS)
        Y, S, N = (eng.stft(a.reshape(R_ * K_, M_, L_)).numpy().reshape(R_, K_, eng.T, eng.F, M_) for a in (y, s, n))
        mask = eng.tf_mask(np.ascontiguousarray(S[:, k, :, :, m]), np.ascontiguousarray(N[:, k, :, :, m]), type='irm1').numpy()
    finally:
        eng.set_lengths(None)
    assert np.array_equal(np.ascontiguousarray(p['Y'].numpy()[:, k, :, :, m]).view(np.uint64), np.ascontiguousarray(Y[:, k, :, :, m]).view(np.uint64)), 'mixture spectrum'
    assert np.array_equal(_bits(p['mask'].numpy()[:, k, :, :, m]), _bits(mask)), 'mask'
    assert np.abs(Y[:, k, :, :, m]).max() > 0 and 0 < mask.max() <= 1
    return True


def expected_files(scene, case, rir_ids, noise, snr_dir, n_mic, save_target=True):
    """The layout of PostGenerator.save_data (post_generator.py:133-166), spelled out: paths relative to the data set's root."""
    files = set()
    for rir in rir_ids:
        for ch in range(1, n_mic + 1):
            for kind, ext in (('wav_processed', 'wav'), ('stft_processed/raw', 'npy')):
                if save_target:
                    files.add(f'{scene}/{case}/{kind}/{snr_dir}/target/{rir}_Ch-{ch}.{ext}')
                files.add(f'{scene}/{case}/{kind}/{snr_dir}/noise/{rir}_{noise}_Ch-{ch}.{ext}')
                files.add(f'{scene}/{case}/{kind}/{snr_dir}/mixture/{rir}_{noise}_Ch-{ch}.{ext}')
            files.add(f'{scene}/{case}/stft_processed/normed/abs/{snr_dir}/mixture/{rir}_{noise}_Ch-{ch}.npy')
            files.add(f'{scene}/{case}/mask_processed/{snr_dir}/{rir}_{noise}_Ch-{ch}.npy')
        files.add(f'{scene}/{case}/log/snrs/dry/{snr_dir}/{rir}_{noise}.npy')
    return files


def files_under(root):
    return {os.path.relpath(os.path.join(d, f), root).replace(os.sep, '/') for d, _, fs in os.walk(root) for f in fs}


def check_round_trip(tmp_path):
    """post_process_rooms -> write_post_dataset -> write_z_dataset -> get_input_lists -> SpectraBank.from_files against from_rooms."""
    from disco_amd.dataset_utils import write_post_dataset
    from disco_amd.dnn.utils import get_input_lists
    from disco_amd.speech_enhancement.z_dataset import write_z_dataset
    root = str(tmp_path)
    assert write_post_dataset(root, 'random', 'train', RIR_IDS, 'ssn', post(), SNR, [0, 6]) == list(RIR_IDS)
    assert files_under(root) == expected_files('random', 'train', RIR_IDS, 'ssn', '0-6', K_ * M_)
    a = np.load(os.path.join(root, 'random/train/stft_processed/raw/0-6/mixture/12_ssn_Ch-3.npy'))
    assert a.dtype == np.complex64 and a.shape == (257, FRAMES[1]), 'the reference holds (F, T), a room has its own frames'
    assert np.load(os.path.join(root, 'random/train/mask_processed/0-6/12_ssn_Ch-3.npy')).shape == (257, FRAMES[1])
    assert np.load(os.path.join(root, 'random/train/log/snrs/dry/0-6/12_ssn.npy')).tolist() == [3.0]
    assert write_post_dataset(root, 'random', 'train', RIR_IDS, 'ssn', post(), SNR, [0, 6]) == [], 'a logged room is skipped'
    o = step1()
    write_z_dataset(os.path.join(root, 'random', 'train', 'stft_z', 'oracle'), RIR_IDS, 'ssn', o['z_y'], o['zn'], snr_range=[[0, 6]])
    z_sigs = ['zs_hat', 'zn_hat']
    lists = get_input_lists(root, RIR_IDS, scenes='random', snr_range=[0, 6], noise_to_get='ssn', ref_channel=REF, z_sigs=z_sigs,
                            mics_per_node=(M_,) * K_, rng=np.random.default_rng(0))
    assert len(lists) == K_ * 4 and all(len(one) == R_ and all(os.path.isfile(f) for f in one) for one in lists)
    from_files = D.SpectraBank.from_files(lists, skip_frames=SKIP, n_nodes=K_, win_len=WIN)
    from_rooms = bank_of(z_sigs)
    assert np.array_equal(from_files.n_frames, from_rooms.n_frames) and from_files.data.shape == from_rooms.data.shape
    is_mag = np.repeat(np.arange(4) < 3, K_)
    return _same_banks(from_rooms.data.cpu().numpy(), from_files.data.numpy(), is_mag, 'files against rooms')


# ---- host only: names and lists ---------------------------------------------------------------------------------------------------------------

def fake_post(R, mics_per_node, T=3, F=2, L=10, seed=0):
    """What post_process_rooms returns, as small host arrays (write_post_dataset takes any container)"""
    rng = np.random.default_rng(seed)
    K, M = len(mics_per_node), mics_per_node[0]
    c = lambda: (rng.standard_normal((R, K, T, F, M)) + 1j * rng.standard_normal((R, K, T, F, M))).astype(np.complex64)
    w = lambda: (0.1 * rng.standard_normal((R, K * M, L))).astype(np.float32)
    return dict(y=w(), s=w(), n=w(), Y=c(), S=c(), N=c(), mask=rng.random((R, K, T, F, M)).astype(np.float32), frames=np.full(R, T), lengths=np.full(R, L),
                mics_per_node=tuple(mics_per_node))


def check_file_names(tmp_path):
    """write_post_dataset's folders and names against the literal layout, for a (2, 2) set and for the reference's four nodes of four; what the
    files hold: (F, T) of the room's own frames, np.abs of the raw mixture, the mask's channel."""
    from disco_amd.dataset_utils import write_post_dataset
    from disco_amd.speech_enhancement.results_io import read_wav
    for mpn, ids, noise, rng_dir, snr_range, target in (((2, 2), (7, 8), 'ssn', '0-6', [0, 6], True), ((4, 4, 4, 4), (10001,), 'fs', '5-15', [5, 15], False)):
        root = os.path.join(str(tmp_path), rng_dir)
        p = fake_post(len(ids), mpn)
        p['frames'][0], p['lengths'][0] = 2, 7
        assert write_post_dataset(root, 'living', 'val', ids, noise, p, 4.5, snr_range, save_target=target) == list(ids)
        assert files_under(root) == expected_files('living', 'val', ids, noise, rng_dir, sum(mpn), save_target=target)
        n_mic, M = sum(mpn), mpn[0]
        ch = n_mic - 1                                                          # counted from 1: node K - 1's microphone M - 2
        k, m = (ch - 1) // M, (ch - 1) % M
        base = os.path.join(root, 'living', 'val')
        raw = np.load(os.path.join(base, 'stft_processed', 'raw', rng_dir, 'mixture', f'{ids[0]}_{noise}_Ch-{ch}.npy'))
        assert raw.dtype == np.complex64 and np.array_equal(raw, p['Y'][0, k, :2, :, m].T)
        mag = np.load(os.path.join(base, 'stft_processed', 'normed', 'abs', rng_dir, 'mixture', f'{ids[0]}_{noise}_Ch-{ch}.npy'))
        assert mag.dtype == np.float32 and np.array_equal(mag, np.abs(raw))
        assert np.array_equal(np.load(os.path.join(base, 'mask_processed', rng_dir, f'{ids[0]}_{noise}_Ch-{ch}.npy')), p['mask'][0, k, :2, :, m].T)
        wav, fs = read_wav(os.path.join(base, 'wav_processed', rng_dir, 'noise', f'{ids[0]}_{noise}_Ch-{ch}.wav'))
        assert fs == 16000 and wav.shape == (7,) and np.abs(wav - p['n'][0, ch - 1, :7]).max() <= 2.0 ** -15
        assert np.load(os.path.join(base, 'log', 'snrs', 'dry', rng_dir, f'{ids[0]}_{noise}.npy')).tolist() == [4.5]
    return True


def check_input_lists():
    from disco_amd.dnn.utils import get_input_lists
    # the reference's set: four nodes of four microphones, channel ref_channel + 4 k
    lists = get_input_lists('/data', [3, 4], ref_channel=2, z_sigs=['zs_hat', 'zn_hat'], rng=np.random.default_rng(0))
    assert len(lists) == 16 and all(len(one) == 2 for one in lists)
    for k in range(4):
        assert lists[k] == [f'/data/random/train/stft_processed/normed/abs/0-6/mixture/{rir}_ssn_Ch-{2 + 4 * k}.npy' for rir in (3, 4)]
        assert lists[4 + k] == [f'/data/random/train/stft_z/oracle/normed/abs/0-6/zs_hat/{rir}_ssn_Node-{k + 1}.npy' for rir in (3, 4)]
        assert lists[8 + k] == [f'/data/random/train/stft_z/oracle/normed/abs/0-6/zn_hat/{rir}_ssn_Node-{k + 1}.npy' for rir in (3, 4)]
        assert lists[12 + k] == [f'/data/random/train/mask_processed/0-6/{rir}_ssn_Ch-{2 + 4 * k}.npy' for rir in (3, 4)]
    # no z signals; another z folder; a ragged array: channel ref_channel + the microphones of the nodes before
    lists = get_input_lists('/d', [9], scenes='meeting', snr_range=[[3, 6], [5, 15]], noise_to_get='it', ref_channel=1, mics_per_node=(2, 3, 1))
    assert lists == [[f'/d/meeting/train/stft_processed/normed/abs/3-6_5-15/mixture/9_it_Ch-{c}.npy'] for c in (1, 3, 6)] + \
        [[f'/d/meeting/train/mask_processed/3-6_5-15/9_it_Ch-{c}.npy'] for c in (1, 3, 6)]
    one = get_input_lists('/d', [9], z_sigs='zs_hat', z_file='crnn', mics_per_node=(2, 2))
    assert one[2] == ['/d/random/train/stft_z/crnn/normed/abs/0-6/zs_hat/9_ssn_Node-1.npy'] and len(one) == 6
    # the draws: per RIR one scene and one noise for all of its files, every choice taken, the same lists from the same generator
    rirs = list(range(1, 201))
    kw = dict(scenes=['random', 'living'], noise_to_get='noit', z_sigs='zn_hat', mics_per_node=(2, 2))
    lists = get_input_lists('/d', rirs, rng=np.random.default_rng(7), **kw)
    assert lists == get_input_lists('/d', rirs, rng=np.random.default_rng(7), **kw) and lists != get_input_lists('/d', rirs, rng=np.random.default_rng(8), **kw)
    seen = set()
    for i, rir in enumerate(rirs):
        parts = [(one[i].split('/')[2], os.path.basename(one[i]).split('_')[1]) for one in lists]
        assert len(set(parts)) == 1 and os.path.basename(lists[0][i]).startswith(f'{rir}_')
        seen.add(parts[0])
    assert seen == {(sc, no) for sc in ('random', 'living') for no in ('ssn', 'fs')}
    assert {os.path.basename(f).split('_')[1] for f in get_input_lists('/d', rirs, noise_to_get='all', rng=np.random.default_rng(1))[0]} == {'ssn', 'it', 'fs'}
    import pytest
    with pytest.raises(ValueError):
        get_input_lists('/d', [1], noise_to_get='babble')
    with pytest.raises(ValueError):
        get_input_lists('/d', [1], ref_channel=3, mics_per_node=(2, 2))
    return True


def check_dset_names():
    import pytest
    from disco_amd.dataset_utils import get_directory_name, get_dset
    assert [get_dset(r) for r in (1, 9999, 10000, 10999, 11000, 11999)] == ['train', 'train', 'val', 'val', 'test', 'test']
    assert [get_dset(r, (5, 3, 2)) for r in (1, 4, 5, 7, 8, 9)] == ['train', 'train', 'val', 'val', 'test', 'test']
    assert get_dset(2, (5, 3, 2), nb_rir=2) == 'train'
    for bad in (dict(rir=0), dict(rir=12000), dict(rir=10, n_samples=(5, 3, 2)), dict(rir=2, n_samples=(5, 3, 2), nb_rir=3)):
        with pytest.raises(ValueError):
            get_dset(**bad)
    assert get_directory_name([0, 6]) == '0-6' and get_directory_name(np.array([5, 15])) == '5-15' and get_directory_name([[0, 6]]) == '0-6'
    assert get_directory_name([[3, 6], [5, 15]]) == '3-6_5-15'
    return True
