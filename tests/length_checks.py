"""Checks of batches whose rooms differ in clip length (disco_set_lengths / Engine.set_lengths): every room of a mixed batch must come out
as if it had been run alone in a context of its own length.  Shared by tests/test_gpu_mixed_lengths.py (MI355X, `-m gpu`) and
tests/test_mixed_lengths_emulated.py (hipemu, reduced sizes); `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library
under test.

The yardstick is the project's own: the float64 oracle run on each room ALONE at its own length (oracle/tango_oracle.py,
oracle/stft_oracle.py), relative error per room and node < 1e-4 on z_y, yf and the time output, masks as
parity_checks.check_tango_end_to_end holds them.

Lengths whose samples are scored against the oracle have L % hop <= hop / 2: nearer to a whole hop librosa's rule divides the last
samples by a window sum that is almost zero (sin^4 of the window's tail) and float32 rounding of the inverse transform is amplified
with them -- in the uniform path just as well.  Lengths beyond that appear where spectra, masks or bit patterns are
compared."""
import numpy as np

import parity_checks as pc
from oracle import mwf_oracle as mo
from oracle import stft_oracle as so
from oracle import tango_oracle as to

relerr = pc.relerr

# rooms 0-5 of the (3, 2) shape (P2 = 4: every room keeps T_r >= 4 P2 + 4 = 20 frames of 256 samples)
LENGTHS_K3M2 = (12288, 8193, 10000, 6272, 5120, 11100)
MODES = ('local', None, 'distant', 'compressed', 'use_oracle_refs', 'use_oracle_zs', 'previous')


def frames_of(L, n_fft):
    return 1 + int(L) // (n_fft // 2)


def scorable(L, n_fft):
    """may the SAMPLES of a clip of this length be scored against the oracle? (see the module docstring)"""
    return int(L) % (n_fft // 2) <= n_fft // 4


def edge_lengths(n_fft, pad_mode='reflect'):
    """(Lmax, lengths): the shortest legal clip, whole hops, one past, half a hop past, one short of a whole hop, a clip that ends in a
    workgroup's first run of frames and one that ends in its last, and Lmax itself -- not sorted."""
    H = n_fft // 2
    Lmax = 37 * H + 100
    shortest = H + 1 if pad_mode == 'reflect' else 1
    return Lmax, (20 * H + 1, shortest, Lmax, 9 * H, 5 * H + 7, 33 * H + H // 2, 12 * H - 1, 36 * H + 3)


def _padded(rng, shape, lengths, fill):
    """random signals of shape (R, ..., Lmax) whose samples at and beyond lengths[r] hold `fill` (a number, NaN, or 'random')"""
    x = rng.standard_normal(shape).astype(np.float32)
    for r, L in enumerate(lengths):
        if fill != 'random':
            x[r, ..., L:] = fill
    return x


# ---- 1 + 2: the transforms at the edges, and the padding is ignored ----------------------------------------------------------------
def check_stft_edges(make_engine, n_fft, pad_mode, chans, seed=0, tol=2e-6):
    Lmax, lens = edge_lengths(n_fft, pad_mode)
    R, H = len(lens), n_fft // 2
    rng = np.random.default_rng(seed)
    x = _padded(rng, (R, chans, Lmax), lens, 'random')
    eng = make_engine(rooms=R, nodes=1, mics=chans, length=Lmax, n_fft=n_fft, pad_mode=pad_mode)
    eng.set_lengths(lens)
    assert np.array_equal(eng.lengths, lens) and np.array_equal(eng.frames, [1 + L // H for L in lens])
    assert eng.T == frames_of(Lmax, n_fft), 'disco_n_frames keeps returning Tmax'
    X = eng.stft(x).numpy()                                                # (R, Tmax, F, chans)
    worst = 0.0
    for r, L in enumerate(lens):
        Tr = frames_of(L, n_fft)
        ref = np.transpose(so.stft(x[r, :, :L], n_fft, H, pad_mode, np.complex128), (2, 1, 0))     # (T_r, F, chans)
        e = pc.maxrel(X[r, :Tr], ref)
        worst = max(worst, e)
        assert e < tol, (r, L, e)
        assert not X[r, Tr:].any(), ('frames beyond T_r must be exact zeros', r, L)
    # the padding is never read: NaN there changes no bit
    xn = x.copy()
    for r, L in enumerate(lens):
        xn[r, :, L:] = np.nan
    Xn = eng.stft(xn).numpy()
    assert np.array_equal(X, Xn), 'samples beyond L_r were read'
    return worst


def check_istft_edges(make_engine, n_fft, seed=1, tol=3e-6):
    Lmax, lens = edge_lengths(n_fft)
    R, H, F = len(lens), n_fft // 2, n_fft // 2 + 1
    Tmax = frames_of(Lmax, n_fft)
    rng = np.random.default_rng(seed)
    Z = (rng.standard_normal((R, Tmax, F)) + 1j * rng.standard_normal((R, Tmax, F))).astype(np.complex64)
    eng = make_engine(rooms=R, nodes=1, mics=1, length=Lmax, n_fft=n_fft)
    eng.set_lengths(lens)
    y = eng.istft(Z).numpy()
    worst = 0.0
    for r, L in enumerate(lens):
        Tr = frames_of(L, n_fft)
        assert not y[r, L:].any(), ('samples beyond L_r must be exact zeros', r, L)
        if scorable(L, n_fft):
            ref = so.istft(np.transpose(Z[r:r + 1, :Tr], (0, 2, 1)), L, n_fft, H, work_dtype=np.float64)[0]
            e = pc.maxrel(y[r, :L], ref)
            worst = max(worst, e)
            assert e < tol, (r, L, e)
    # frames beyond T_r do not exist: NaN there changes no bit
    Zn = Z.copy()
    for r, L in enumerate(lens):
        Zn[r, frames_of(L, n_fft):] = np.nan
    assert np.array_equal(y, eng.istft(Zn).numpy()), 'frames beyond T_r were read'
    # round trip on real signals, every length
    x = _padded(rng, (R, 1, Lmax), lens, np.nan)
    xr = eng.istft(eng.stft(x).reshape(R, Tmax, F)).numpy()
    for r, L in enumerate(lens):
        if scorable(L, n_fft):
            assert float(np.abs(xr[r, :L] - x[r, 0, :L]).max()) < 2e-5, (r, L)
    return worst


def check_mask_edges(make_engine, n_fft, seed=2, masks=('irm1', 'irm2', 'iam1', 'ibm1')):
    """disco_mask_oracle with TWO signals per room (signal g belongs to room g / 2)"""
    Lmax, lens = edge_lengths(n_fft)
    R, H = len(lens), n_fft // 2
    rng = np.random.default_rng(seed)
    lens2 = [L for L in lens for _ in range(2)]
    s = _padded(rng, (2 * R, Lmax), lens2, np.nan)
    n = _padded(rng, (2 * R, Lmax), lens2, np.nan)
    s[:, :100] = 0
    worst = 0.0
    for mask in masks:
        eng = make_engine(rooms=R, nodes=1, mics=1, length=Lmax, n_fft=n_fft, mask=mask)
        eng.set_lengths(lens)
        m = eng.mask_oracle(s, n).numpy()                                  # (2 R, Tmax, F)
        assert np.isfinite(m).all()
        errs = []
        for g, L in enumerate(lens2):
            Tr = frames_of(L, n_fft)
            assert not m[g, Tr:].any(), ('masks of frames beyond T_r are forced to zero', mask, g, L)
            S = so.stft(s[g:g + 1, :L], n_fft, H, 'reflect', np.complex128)
            Nn = so.stft(n[g:g + 1, :L], n_fft, H, 'reflect', np.complex128)
            with np.errstate(all='ignore'):
                ref = np.transpose(mo.tf_mask(S, Nn, type=mask), (0, 2, 1)).astype(np.float64)[0]
            if mask.startswith('ibm'):
                assert np.mean(m[g, :Tr] != ref) < 1e-3
            else:
                ok = np.isfinite(ref)
                errs.append(np.abs(m[g, :Tr][ok] - ref[ok]) / (1.0 + np.abs(ref[ok])))
        if errs:
            # as parity_checks.check_masks: the bulk (99.9th percentile) and the tail (max) over the valid part of the WHOLE batch -- the
            # percentile of a two-frame clip taken alone would be its maximum, which that check holds to the looser bound
            err = np.concatenate(errs)
            e = float(np.percentile(err, 99.9))
            worst = max(worst, e)
            assert e < 2e-5 and float(err.max()) < 5e-3, (mask, e, float(err.max()))
        import pytest
        from disco_amd.engine import DiscoError
        with pytest.raises(DiscoError, match='multiple'):                  # n_sig must be a multiple of the rooms
            eng.mask_oracle(s[:2 * R - 1], n[:2 * R - 1])
    return worst


def check_cov_mean(make_engine, K=2, M=2, n_fft=512, seed=3):
    """disco_cov_masked / disco_stft_cov_fused hand out the mean over a room's OWN frames"""
    lens = (6272, 5120, 7000)
    Lmax, R = 7168, 3
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=Lmax, n_fft=n_fft)
    eng.set_lengths(lens)
    y = _padded(rng, (R, K, M, Lmax), lens, np.nan)
    mask = rng.uniform(0.05, 0.95, (R, K, eng.T, eng.F)).astype(np.float32)
    X, Rss_f, Rnn_f = eng.stft_cov_fused(y, mask)
    Rss, Rnn = eng.cov_masked(X, mask)
    Xh = X.numpy()
    for r, L in enumerate(lens):
        Tr = frames_of(L, n_fft)
        assert not Xh[r, :, Tr:].any()
        rs, rn = pc.oracle_cov(Xh[r:r + 1, :, :Tr], mask[r:r + 1, :, :Tr])
        for got_s, got_n in ((Rss, Rnn), (Rss_f, Rnn_f)):
            assert relerr(got_s.numpy()[r], rs[0]) < 2e-6 and relerr(got_n.numpy()[r], rn[0]) < 2e-6, (r, L)
    return True


# ---- 3, 6: the whole path -----------------------------------------------------------------------------------------------------------
def mixed_rooms(K, M, lengths, Lmax, fill=np.nan, first_room=0):
    """rooms from synth.make_room_numpy, each generated AT ITS OWN LENGTH and copied into the rectangular batch -> y, s, n (R, K, M, Lmax)
    with `fill` beyond each room's clip, and the list of the per-room (y, s, n) at their own lengths"""
    from disco_amd import synth
    R = len(lengths)
    ysn = np.full((3, R, K, M, Lmax), fill, np.float32)
    own = []
    for r, L in enumerate(lengths):
        room = synth.make_room_numpy(first_room + r, K=K, M=M, L=int(L))[:3]
        own.append(room)
        for i in range(3):
            ysn[i, r, :, :, :L] = room[i]
    return ysn[0], ysn[1], ysn[2], own


def _oracle_room(room, n_fft, mask='irm1', iters=1, mask_for_z='local'):
    y, s, n = room
    return to.offline_tango_vec(y, s, n, vads=[mask, mask], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh',
                                extra_iters=iters - 1, mask_for_z=mask_for_z)


def check_whole_path(make_engine, K, M, lengths, n_fft=512, Lmax=None, staged_step2=False, tuning=None, overlap=None, iters=0, tol=1e-4,
                     options=None, want_stage=None, alone=True):
    """disco_mask_oracle + disco_tango_enhance (iters = 0; with and without z / yf requested) or disco_tango_enhance_iterated (iters >= 1)
    on a mixed batch whose padding holds NaN, against the float64 oracle of every room alone at its own length; exact zeros in the padding
    of every output; the same bits with other (finite) caller masks in the padding frames and with other samples in the padding; and
    every room against the same room in a one-room engine of its own length (`alone`)."""
    R = len(lengths)
    Lmax = Lmax or max(lengths)
    H = n_fft // 2
    y, s, n, own = mixed_rooms(K, M, lengths, Lmax)

    def engine(rooms, length):
        e = make_engine(rooms=rooms, nodes=K, mics=M, length=length, n_fft=n_fft, staged_step2=staged_step2)
        if tuning is not None:
            e.set_tuning(*tuning)
        for key, v in (options or {}).items():
            e.set_option(key, v)
        return e

    eng = engine(R, Lmax)
    if overlap is not None:
        eng.set_option('overlap_solves', overlap)
    eng.set_lengths(lengths)
    T, F = eng.T, eng.F

    def run(e, y_, s_, n_, mask=None, workspace=None):
        Rr, L_ = y_.shape[0], y_.shape[-1]
        m = mask if mask is not None else e.mask_oracle(s_[:, :, 0].reshape(Rr * K, L_), n_[:, :, 0].reshape(Rr * K, L_)).reshape(Rr, K, e.T, e.F)
        if iters:
            out, yf = e.tango_enhance_iterated(y_, m, iters=iters)
            return dict(m=m.numpy() if hasattr(m, 'numpy') else m, out=out.numpy(), yf=yf.numpy())
        out, z, yf = e.tango_enhance(y_, m, workspace=workspace)
        out_enh = e.tango_enhance(y_, m, want_z=False, want_yf=False, workspace=workspace)[0].numpy()
        return dict(m=m.numpy() if hasattr(m, 'numpy') else m, out=out.numpy(), z=z.numpy(), yf=yf.numpy(), out_enh=out_enh)

    if want_stage:
        eng.stage_timing(True)
    got = run(eng, y, s, n)
    if want_stage:
        stages = set(eng.stage_report())
        eng.stage_timing(False)
        assert want_stage in stages, (want_stage, stages)
    errs = {}

    def worst(key, v):
        errs[key] = max(errs.get(key, 0.0), float(v))

    for r, L in enumerate(lengths):
        assert scorable(L, n_fft), ('samples are scored: L % hop <= hop / 2', L)
        Tr = 1 + L // H
        o = _oracle_room(own[r], n_fft, iters=max(iters, 1))
        for key in got:
            pad = got[key][r, :, L:] if key.startswith('out') else got[key][r, :, Tr:]
            assert not pad.any() and np.isfinite(got[key][r]).all(), ('padding must be exact zeros', key, r)
        for k in range(K):
            dm = np.abs(got['m'][r, k, :Tr].T - o['masks_z'][k])
            worst('mask', np.percentile(dm, 99.9))
            worst('mask_max', dm.max())
            if 'z' in got:
                worst('z_y', relerr(got['z'][r, k, :Tr].T, o['z_y'][k]))
            worst('yf', relerr(got['yf'][r, k, :Tr].T, o['yf'][k]))
            t_ref = so.istft(o['yf'][k], L, n_fft, H, work_dtype=np.float64)
            worst('out', relerr(got['out'][r, k, :L], t_ref))
            if 'out_enh' in got:
                worst('out_enhanced_only', relerr(got['out_enh'][r, k, :L], t_ref))
    print('mixed lengths vs oracle', (K, M, n_fft, staged_step2, overlap, iters), errs)
    assert errs['mask'] < 2e-5 and errs['mask_max'] < 5e-3, errs
    assert all(errs[k] < tol for k in ('z_y', 'yf', 'out', 'out_enhanced_only') if k in errs), errs

    # the padding is ignored: other samples there, and other finite mask values in the frames beyond T_r, change no bit
    y2, s2, n2, _ = mixed_rooms(K, M, lengths, Lmax, fill=0.25)
    m2 = got['m'].copy()
    for r, L in enumerate(lengths):
        m2[r, :, 1 + L // H:] = 0.37
    again = run(eng, y2, s2, n2, mask=m2)
    for key in got:
        if key != 'm':
            assert np.array_equal(got[key], again[key]), ('the padding was read', key)
    # nor does anything depend on what the workspace held (frames of X that a route leaves unwritten are read by nobody)
    if not iters:
        ws = eng.to_device(np.full(eng.workspace_bytes(), 0xFF, np.uint8), np.uint8)[1]          # all-ones bytes: NaN everywhere
        dirty = run(eng, y, s, n, mask=got['m'], workspace=ws)
        for key in got:
            if key != 'm':
                assert np.array_equal(got[key], dirty[key]), ('the result depends on the previous content of the workspace', key)

    # alone equals batched within rounding (both within tol of the oracle => within 2 tol of each other); compared through the spectra
    if alone:
        for r, L in enumerate(lengths):
            solo = engine(1, int(L))
            one = run(solo, *(a[None] for a in own[r]))
            Tr = 1 + L // H
            for key in ('z', 'yf'):
                if key in got:
                    for k in range(K):
                        worst('alone_' + key, relerr(got[key][r, k, :Tr], one[key][0, k]))
        print('alone vs batched', {k: v for k, v in errs.items() if k.startswith('alone')})
        assert all(v < 2 * tol for k, v in errs.items() if k.startswith('alone')), errs
    return errs


def check_alone_equals_batched_near_whole_hop(make_engine, K=3, M=2, n_fft=512, tol=1e-4):
    """lengths with L % hop > hop / 2, where samples are not scored: the spectra of a room of the mixed batch against the same room alone"""
    lengths = (6143, 11007, 8000)
    H = n_fft // 2
    y, s, n, own = mixed_rooms(K, M, lengths, 11264)
    eng = make_engine(rooms=3, nodes=K, mics=M, length=11264, n_fft=n_fft)
    eng.set_lengths(lengths)
    m = eng.mask_oracle(s[:, :, 0].reshape(3 * K, -1), n[:, :, 0].reshape(3 * K, -1)).reshape(3, K, eng.T, eng.F)
    out, z, yf = eng.tango_enhance(y, m)
    worst = 0.0
    for r, L in enumerate(lengths):
        solo = make_engine(rooms=1, nodes=K, mics=M, length=L, n_fft=n_fft)
        yr, sr, nr = (a[None] for a in own[r])
        m1 = solo.mask_oracle(sr[0, :, 0], nr[0, :, 0]).reshape(1, K, solo.T, solo.F)
        _, z1, yf1 = solo.tango_enhance(yr, m1)
        Tr = 1 + L // H
        assert not out.numpy()[r, :, L:].any()
        for a, b in ((z, z1), (yf, yf1)):
            worst = max(worst, max(relerr(a.numpy()[r, k, :Tr], b.numpy()[0, k]) for k in range(K)))
    print('alone vs batched, L % hop > hop / 2:', worst)
    assert worst < 2 * tol, worst
    return worst


# ---- 4: disco_tango_reference --------------------------------------------------------------------------------------------------------
def check_reference_outputs(make_engine, K=3, M=2, lengths=LENGTHS_K3M2, n_fft=512, modes=MODES, tol=1e-4):
    """all nine outputs, every mask_for_z mode, steps = 3 and steps = 1 then 2, per room against the oracle at the room's own length"""
    Lmax, R, H = max(lengths), len(lengths), n_fft // 2
    y, s, n, own = mixed_rooms(K, M, lengths, Lmax)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=Lmax, n_fft=n_fft)
    eng.set_lengths(lengths)
    out = {}
    y, s, n = (eng.to_device(a, np.float32)[1] for a in (y, s, n))       # device resident: steps = 2 continues from the SAME arrays
    for mode in modes:
        got = {nm: b.numpy() for nm, b in eng.tango_reference(y, s, n, mask_for_z=mode).items()}
        two = {nm: b.numpy() for nm, b in eng.tango_reference(y, s, n, mask_for_z=mode, steps=1).items()}
        two.update({nm: b.numpy() for nm, b in eng.tango_reference(y, s, n, mask_for_z=mode, steps=2).items()})
        assert set(got) == set(two) and all(np.array_equal(got[nm], two[nm]) for nm in got), ('steps = 1 then 2 differs from steps = 3', mode)
        e = 0.0
        for r, L in enumerate(lengths):
            Tr = 1 + L // H
            o = _oracle_room(own[r], n_fft, mask_for_z=mode)
            for key in ('z_y', 'z_s', 'z_n', 'zn', 'yf', 'sf', 'nf', 'masks_z', 'mask_w'):
                assert not got[key][r, :, Tr:].any() and np.isfinite(got[key][r]).all(), ('padding must be exact zeros', mode, key, r)
                for k in range(K):
                    if 'mask' in key:
                        dm = np.abs(got[key][r, k, :Tr].T - o[key][k])
                        assert float(np.percentile(dm, 99.9)) < 2e-5 and float(dm.max()) < 5e-3, (mode, key, r, k)
                    else:
                        e = max(e, relerr(got[key][r, k, :Tr].T, o[key][k]))
        out[mode] = e
        assert e < tol, (mode, e)
    print('tango_reference, mixed lengths:', out)
    return out


# ---- 5: the uniform batch is untouched -----------------------------------------------------------------------------------------------
def check_uniform_untouched(make_engine, K=4, M=4, L=9000, R=3, n_fft=512, tuning=(40, 1, 1, 16)):
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)

    def run(e):
        m = e.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, e.T, e.F)
        out, z, yf = e.tango_enhance(y, m)
        out_enh = e.tango_enhance(y, m, want_z=False, want_yf=False)[0]
        Rss, Rnn = e.cov_masked(e.stft(y.reshape(R * K, M, L)).reshape(R, K, e.T, e.F, M), m)
        return [a.numpy() for a in (m, out, z, yf, out_enh, Rss, Rnn)]

    def engine():
        e = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        e.set_tuning(*tuning)
        return e

    fresh = run(engine())
    eng = engine()
    eng.set_lengths([L] * R)
    full = run(eng)
    eng.set_lengths(None)
    none = run(eng)
    for name, a, b, c in zip(('mask', 'out', 'z_y', 'yf', 'out_enhanced_only', 'Rss', 'Rnn'), fresh, full, none):
        assert np.array_equal(a, b), ('lengths == Lmax differs from the uniform batch', name)
        assert np.array_equal(a, c), ('set_lengths(None) does not restore the uniform batch', name)
    return True


# ---- 8: refusals and arguments -------------------------------------------------------------------------------------------------------
def check_refusals(make_engine, lib_error, K=2, M=2, n_fft=512):
    import pytest
    R, Lmax, H = 2, 4096, n_fft // 2
    eng = make_engine(rooms=R, nodes=K, mics=M, length=Lmax, n_fft=n_fft)
    good = [3000, 4096]
    eng.set_lengths(good)
    for bad in ([3000], [3000, 4096, 4096], [0, 4096], [H, 4096], [3000, Lmax + 1]):
        with pytest.raises(lib_error, match='disco_set_lengths'):
            eng.set_lengths(bad)
        assert np.array_equal(eng.lengths, good), 'a refused call must leave the previous lengths in force'
    rng = np.random.default_rng(5)
    x = rng.standard_normal((R, 1, Lmax)).astype(np.float32)
    X = eng.stft(x).numpy()
    assert not X[0, 1 + 3000 // H:].any() and X[1, -1].any(), 'the previous lengths are still what the kernels see'
    const = make_engine(rooms=R, nodes=K, mics=M, length=Lmax, n_fft=n_fft, pad_mode='constant')
    const.set_lengths([1, H])                                              # legal with constant padding
    with pytest.raises(lib_error, match='disco_set_lengths'):
        const.set_lengths([0, H])
    # entry points that do not take lengths say so and touch nothing
    T, F = eng.T, eng.F
    Xc = (rng.standard_normal((R, K, T, F, M)) + 1j * rng.standard_normal((R, K, T, F, M))).astype(np.complex64)
    mask = rng.uniform(0.1, 0.9, (R, K, T, F)).astype(np.float32)
    y = rng.standard_normal((R, K, M, Lmax)).astype(np.float32)
    lib = eng.lib
    sentinel = np.float32(-7.25)

    def untouched(shape, dtype, call):
        buf = eng.to_device(np.full(shape, sentinel, dtype), dtype)[1]
        rc = call(buf)
        assert rc == -2, rc                                                # DISCO_E_UNSUPPORTED
        assert 'lengths' in lib.disco_last_error(eng.ctx).decode()
        assert (buf.numpy() == dtype(sentinel)).all(), 'a refused call wrote to its output'

    px, pm, py = eng.to_device(Xc, np.complex64), eng.to_device(mask, np.float32), eng.to_device(y, np.float32)
    untouched((R, K, T, F), np.complex64,
              lambda b: lib.disco_online_mwf(eng.ctx, px[0], None, pm[0], M, 0.95, 1.0, 1, 1e-3, b.ptr, None, None))
    untouched((R, K, Lmax), np.float32,
              lambda b: lib.disco_tango_online(eng.ctx, py[0], pm[0], pm[0], 0.95, 1, 1e-3, b.ptr, None, None, None, 0, None))
    untouched((R * K, T, F), np.float32, lambda b: lib.disco_mask_ivad(eng.ctx, py[0], R * K, b.ptr, None))
    with pytest.raises(lib_error, match='lengths'):
        eng.online_stream().push(y[..., :2 * H], mask[:, :, :2])
    with pytest.raises(lib_error, match='lengths'):
        eng.set_node_shard(0, 1)
    assert (eng.k0, eng.Kl) == (0, K)
    shard = make_engine(rooms=R, nodes=K, mics=M, length=Lmax, n_fft=n_fft)
    shard.set_node_shard(0, 1)
    with pytest.raises(lib_error, match='lengths'):
        shard.set_lengths(good)
    # and take them again once the lengths are gone
    eng.set_lengths(None)
    eng.mask_ivad(y[:, :, 0].reshape(R * K, Lmax))
    return True


# ---- 9: the Python surface -----------------------------------------------------------------------------------------------------------
NAMES = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']


def check_python_surface(lengths=(8193, 6272, 10000), K=3, M=2):
    """offline_tango_rooms on rooms of different lengths: the reference's 9-tuples per room against the oracle, and against separate
    offline_tango calls"""
    import pytest
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango, offline_tango_batched, offline_tango_rooms
    rooms = [synth.make_room_numpy(r, K=K, M=M, L=L)[:3] for r, L in enumerate(lengths)]
    res = offline_tango_rooms(rooms, vads='irm1')
    assert len(res) == len(rooms)
    worst = {'oracle': 0.0, 'separate': 0.0}
    for r, (L, room) in enumerate(zip(lengths, rooms)):
        Tr = 1 + L // 256
        o = to.as_reference_tuple(to.offline_tango_vec(*room, vads=['irm1', 'irm1'], precision='f64', solver='eigh'))
        sep = offline_tango(*room, vads=['irm1', 'irm1'])
        for i, nm in enumerate(NAMES):
            for k in range(K):
                assert res[r][i][k].shape == (257, Tr), (nm, res[r][i][k].shape)
                e = relerr(res[r][i][k], o[i][k])
                assert e < (2e-5 if 'mask' in nm else 1e-4), (r, nm, k, e)
                worst['oracle'] = max(worst['oracle'], e)
                e2 = relerr(res[r][i][k], sep[i][k])
                assert e2 < 2e-4, (r, nm, k, e2)
                worst['separate'] = max(worst['separate'], e2)
    y = np.zeros((2, K, M, 8192), np.float32)
    with pytest.raises(NotImplementedError, match='lengths'):
        offline_tango_batched(y, y, y, vads='ivad', lengths=[8192, 6000])
    with pytest.raises(ValueError, match=r'\(3, 2\).*\(2, 2\)'):
        offline_tango_rooms([rooms[0], tuple(a[:2] for a in rooms[1])])
    # the cached engines are left without lengths
    d = offline_tango_batched(*(np.stack([a[..., :6272] for a in room3]) for room3 in zip(*rooms)))
    assert d['yf'][0, :, -1].any()
    print('offline_tango_rooms:', worst)
    return worst
