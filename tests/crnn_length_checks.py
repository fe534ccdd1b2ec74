"""Checks of CRNN-mask batches whose rooms differ in clip length: the three helper kernels behind disco_crnn_features_rooms,
disco_crnn_windows_rooms and disco_crnn_expand_rows (taking a bound library and a torch device, as parity_checks.check_crnn_features does),
CRNN.predict_masks(..., frames=...), and the two routes (dnn/inloop.py:tango_enhance_dnn, speech_enhancement/tango.py).  Shared by
tests/test_crnn_lengths_cpu.py, tests/test_crnn_lengths_emulated.py (hipemu) and tests/test_gpu_crnn_lengths.py (MI355X).

The rule everything is held to: every room of a mixed batch comes out as if it had been run alone at its own length."""
import numpy as np

import parity_checks as pc

W, FY = 15, 4                                   # frames and frequency cells of one window of the recurrent layer's input
SENTINEL = -7.25
CRNN_TOL = 1e-4                                 # enhanced signals against the float64 oracle (tests/test_gpu_crnn_inloop.py)
MASK1_TOL, MASK2_TOL = 2e-4, 2e-3               # step-1 / step-2 masks against the float64 network on the oracle's spectra (same file)
ALONE_TOL = 2e-5                                # float32 predict_masks of two batch shapes (test_predict_masks_float32_vs_float64_production_shape)

# The rooms of the whole-path checks (synth.make_room_numpy(r, L=LENGTHS[r])): one at Lmax, one a whole number of hops (16384 = 64 x 256), two
# others; L % 256 <= 128 (length_checks.scorable) and L >= 16000 for all.  No value had to be replaced: each room alone, on the uniform path, is
# within CRNN_TOL of the oracle with the seeded networks below (check_in_loop(..., alone_only=True): worst 7.3e-6 over the five cases).
LENGTHS = (20000, 24100, 16384, 17500)


def rand_model(n_ch, seed, device, out_gain=40.0):
    """tests/test_gpu_crnn_inloop.py:_rand_model: BatchNorm statistics spread, output weights x 40 (masks spread over (0, 1): masks stuck
    near 0.5 would make Rss ~ Rnn, a degenerate eigenproblem no implementation can reproduce tightly).
    out_gain=1: output weights of their initial scale, for the float32-against-float64 checks of the network alone.  Their bar, 2e-5, is the one
    float32 predict_masks is held to on TRAINED weights; the x 40 multiplies the rounding error in front of the sigmoid by 40 and nothing in those
    checks needs it (with it the UNCHANGED rectangular float32 path is 2.1e-5 from float64 on a 40-frame item of the 3-channel network, the
    compacted path 2.2e-5 on the same item; without it both are 6e-7)."""
    import torch
    from torch import nn
    from disco_amd.dnn.crnn import build_crnn
    torch.manual_seed(seed)
    m = build_crnn(n_ch=n_ch)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
    with torch.no_grad():
        m.ff.layers[0].weight.mul_(out_gain)
    return m.to(device).eval()


def _bits(t):
    import torch
    return t.contiguous().cpu().view(torch.int32)


def _dev_ints(values, dtype, device):
    import torch
    return torch.tensor(list(values), dtype=dtype).to(device)


def _row0(frames_sig):
    return np.concatenate(([0], np.cumsum(frames_sig)))[:-1]


# ---- disco_crnn_features_rooms -------------------------------------------------------------------------------------------------------
def check_features_rooms(lib, device, R, K, M, T, F, frame_sets):
    """Rows t < T_r bit-equal to disco_crnn_features on the same inputs, every other element +0.0; the inputs hold NaN, inf and values
    outside [lo, hi] in frames that exist, and nothing but such values in the frames beyond T_r."""
    import torch
    from disco_amd.dnn.crnn import STFT_MAX, STFT_MIN
    g = torch.Generator().manual_seed(31)
    X0 = torch.view_as_complex(torch.randn((R, K, T, F, M, 2), generator=g)).contiguous()
    z0 = torch.view_as_complex(torch.randn((R, K, T, F, 2), generator=g)).contiguous()
    garbage = [complex(float('nan'), 1.0), complex(float('inf'), 0.0), complex(0.0, float('-inf')), complex(5e3, 5e3), complex(1e-9, 0.0)]
    n_calls = 0
    for frames in frame_sets:
        assert len(frames) == R and all(1 <= v <= T for v in frames)
        X, z = X0.clone(), z0.clone()
        for r, Tr in enumerate(frames):
            for i, v in enumerate(garbage):                         # frame 0 exists in every room
                X[r, i % K, 0, i % F, :] = v
                z[r, (i + 1) % K, 0, (i + 2) % F] = v
                X[r, :, Tr:, i::len(garbage)] = v                   # and nothing else beyond T_r
                z[r, :, Tr:, i::len(garbage)] = v
        Xd, zd, fd = X.to(device), z.to(device), _dev_ints(frames, torch.int32, device)
        for with_z in (False, True):
            for mic, pad in ((M - 1, (10, 10)), (0, (17, 3))):
                C_, Tp = (K if with_z else 1), pad[0] + T + pad[1]
                zp = zd.data_ptr() if with_z else None
                rect = torch.empty((R, K, C_, Tp, F), dtype=torch.float32, device=device)
                got = torch.full((R, K, C_, Tp, F), SENTINEL, dtype=torch.float32, device=device)
                assert lib.disco_crnn_features(None, Xd.data_ptr(), zp, R, K, M, T, F, mic, pad[0], pad[1], STFT_MIN, STFT_MAX, rect.data_ptr(),
                                               pc._stream(Xd)) == 0
                assert lib.disco_crnn_features_rooms(None, Xd.data_ptr(), zp, R, K, M, T, F, mic, pad[0], pad[1], STFT_MIN, STFT_MAX, fd.data_ptr(),
                                                     got.data_ptr(), pc._stream(Xd)) == 0
                pc._sync(Xd)
                rect, got = rect.cpu(), got.cpu()
                for r, Tr in enumerate(frames):
                    what = (frames, with_z, mic, pad, r)
                    assert torch.equal(_bits(got[r, :, :, pad[0]:pad[0] + Tr]), _bits(rect[r, :, :, pad[0]:pad[0] + Tr])), what
                    assert not _bits(got[r, :, :, :pad[0]]).any() and not _bits(got[r, :, :, pad[0] + Tr:]).any(), ('not +0.0', what)
                    if Tr < T:                                      # the rectangular entry clips the garbage there: NaN passes, the rest is >= lo
                        assert bool((rect[r, :, :, pad[0] + Tr:pad[0] + T] != 0).all())
                    assert bool(torch.isnan(got[r, :, 0, pad[0]]).any()) and float(got[r].nan_to_num(0.0).max()) == float(np.float32(STFT_MAX))
                n_calls += 1
    # refused, not mis-computed: every bad argument of the rectangular entry, and frames == NULL
    X, z, fd = X0.to(device), z0.to(device), _dev_ints([T] * R, torch.int32, device)
    out = torch.full((R * K, K, T + 20, F), SENTINEL, dtype=torch.float32, device=device)
    good = dict(X=X.data_ptr(), Z=z.data_ptr(), R=R, K=K, M=M, T=T, F=F, mic=0, pad_lo=10, pad_hi=10, lo=STFT_MIN, hi=STFT_MAX, frames=fd.data_ptr(),
                out=out.data_ptr())
    bad = [dict(X=None), dict(out=None), dict(frames=None), dict(R=0), dict(K=0), dict(M=0), dict(T=0), dict(F=0), dict(mic=-1), dict(mic=M),
           dict(pad_lo=-1), dict(pad_hi=-1), dict(lo=2.0, hi=1.0), dict(lo=float('nan'))]
    for change in bad:
        a = dict(good, **change)
        rc = lib.disco_crnn_features_rooms(None, a['X'], a['Z'], a['R'], a['K'], a['M'], a['T'], a['F'], a['mic'], a['pad_lo'], a['pad_hi'], a['lo'],
                                           a['hi'], a['frames'], a['out'], None)
        assert rc == -1, (change, rc)
    pc._sync(out)
    assert bool((out == SENTINEL).all()), 'a refused call wrote to its output'
    return n_calls


# ---- disco_crnn_windows_rooms --------------------------------------------------------------------------------------------------------
def _windows_rooms(lib, feat, T, n_keep, frames_sig, extra_rows=1, n_rows=None):
    import torch
    nb, C, Tp, _ = feat.shape
    N = int(np.sum(frames_sig))
    out = torch.full((N + extra_rows, n_keep), SENTINEL, dtype=torch.float32, device=feat.device)
    fd, rd = _dev_ints(frames_sig, torch.int32, feat.device), _dev_ints(_row0(frames_sig), torch.int64, feat.device)
    rc = lib.disco_crnn_windows_rooms(None, feat.data_ptr(), nb, C, Tp, T, W, n_keep, fd.data_ptr(), rd.data_ptr(), out.data_ptr(),
                                      N if n_rows is None else n_rows, pc._stream(feat))
    assert rc == 0, rc
    pc._sync(feat)
    return out.cpu()


def check_windows_rooms(lib, device, nb=3, C=2, T=6, frame_sets=((6, 1, 4), (6, 6, 6)), n_keeps=(4, 60, 120)):
    """Every compacted row bit-equal to the row disco_crnn_windows writes for that (b, t); one sentinel row past n_rows stays untouched;
    with all frames equal to T the whole output is the rectangular kernel's."""
    import torch
    g = torch.Generator().manual_seed(17)
    Tp = T + W - 1
    feat = torch.randn((nb, C, Tp, FY), generator=g)
    feat[0, 0, 2, 1], feat[1, C - 1, 0, 0] = float('nan'), float('inf')
    fd = feat.to(device)
    for n_keep in n_keeps:
        rect = torch.empty((nb * T, n_keep), dtype=torch.float32, device=device)
        assert lib.disco_crnn_windows(None, fd.data_ptr(), nb, C, Tp, T, W, n_keep, rect.data_ptr(), pc._stream(fd)) == 0
        pc._sync(fd)
        rect = rect.cpu()
        for frames_sig in frame_sets:
            got = _windows_rooms(lib, fd, T, n_keep, frames_sig)
            N, row0 = int(np.sum(frames_sig)), _row0(frames_sig)
            for b, Tb in enumerate(frames_sig):
                assert torch.equal(_bits(got[row0[b]:row0[b] + Tb]), _bits(rect[b * T:b * T + Tb])), (n_keep, frames_sig, b)
            assert bool((got[N:] == SENTINEL).all()), 'wrote past n_rows'
            if all(v == T for v in frames_sig):
                assert torch.equal(_bits(got[:N]), _bits(rect))
        # rows that the caller's buffer does not have are skipped, not written
        short = _windows_rooms(lib, fd, T, n_keep, frame_sets[0], n_rows=int(np.sum(frame_sets[0])) - 2, extra_rows=0)
        assert bool((short[-2:] == SENTINEL).all()) and not bool((short[:-2] == SENTINEL).any())
    # refused, not mis-computed
    feat = torch.zeros((1, 3, 20, 4), device=device)
    out = torch.full((64, 128), SENTINEL, dtype=torch.float32, device=device)
    fs, r0 = _dev_ints([6], torch.int32, device), _dev_ints([0], torch.int64, device)
    f, o, fp, rp = feat.data_ptr(), out.data_ptr(), fs.data_ptr(), r0.data_ptr()
    call = lib.disco_crnn_windows_rooms
    assert call(None, None, 1, 2, 20, 6, W, 120, fp, rp, o, 6, None) == -1             # null pointers
    assert call(None, f, 1, 2, 20, 6, W, 120, None, rp, o, 6, None) == -1
    assert call(None, f, 1, 2, 20, 6, W, 120, fp, None, o, 6, None) == -1
    assert call(None, f, 1, 2, 20, 6, W, 120, fp, rp, None, 6, None) == -1
    assert call(None, f, 1, 2, 20, 6, W, 6, fp, rp, o, 6, None) == -1                  # n_keep % 4
    assert call(None, f, 1, 2, 20, 6, W, 124, fp, rp, o, 6, None) == -1                # n_keep > C W 4
    assert call(None, f, 1, 2, 20, 7, W, 120, fp, rp, o, 6, None) == -1                # Tp < T + W - 1
    assert call(None, f + 4, 1, 2, 19, 5, W, 120, fp, rp, o, 5, None) == -1            # feat off 16-byte alignment
    assert call(None, f, 1, 2, 20, 6, W, 120, fp, rp, o + 4, 6, None) == -1            # out off 16-byte alignment
    assert call(None, f, 1, 2, 20, 6, W, 120, fp, rp, o, 0, None) == -1                # no rows
    assert call(None, f, 0, 2, 20, 6, W, 120, fp, rp, o, 6, None) == -1
    pc._sync(out)
    assert bool((out == SENTINEL).all()), 'a refused call wrote to its output'
    assert call(None, f, 1, 2, 20, 6, W, 120, fp, rp, o, 6, None) == 0                  # (and the same call with good arguments is taken)
    pc._sync(out)
    return True


# ---- disco_crnn_expand_rows ----------------------------------------------------------------------------------------------------------
def _expand_ref(rows, B, T, frames_sig):
    import torch
    out = torch.zeros((B, T, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    b_idx = torch.from_numpy(np.repeat(np.arange(B), frames_sig)).to(rows.device)
    t_idx = torch.from_numpy(np.concatenate([np.arange(n) for n in frames_sig])).to(rows.device)
    out[b_idx, t_idx] = rows
    return out


def check_expand_rows(lib, device, Fs=(17, 257), T=6, frame_sets=((6, 1, 4), (6, 6, 6))):
    """Existing rows bit-equal, every other element +0.0, no sentinel survives in `out` and the floats around it stay; with `out` on a
    16-byte boundary (16-byte stores) and 4 bytes off it (single stores)."""
    import torch
    g = torch.Generator().manual_seed(23)
    for F in Fs:
        for frames_sig in frame_sets:
            B, N = len(frames_sig), int(np.sum(frames_sig))
            rows = torch.randn((N, F), generator=g)
            rows[0, 0], rows[N - 1, F - 1] = float('nan'), float('-inf')
            rd = rows.to(device)
            fd, r0 = _dev_ints(frames_sig, torch.int32, device), _dev_ints(_row0(frames_sig), torch.int64, device)
            want = _expand_ref(rows, B, T, frames_sig)
            for off in (4, 5):                                      # floats before `out` in its buffer: aligned / 4 bytes off
                buf = torch.full((off + B * T * F + 3,), SENTINEL, dtype=torch.float32, device=device)
                assert buf.data_ptr() % 16 == 0
                rc = lib.disco_crnn_expand_rows(None, rd.data_ptr(), N, B, T, F, fd.data_ptr(), r0.data_ptr(), buf.data_ptr() + 4 * off, pc._stream(rd))
                assert rc == 0, rc
                pc._sync(rd)
                buf = buf.cpu()
                got = buf[off:off + B * T * F].view(B, T, F)
                assert torch.equal(_bits(got), _bits(want)), (F, frames_sig, off)
                assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + B * T * F:] == SENTINEL).all()), 'wrote outside out'
    rows, out = torch.zeros((6, 17), device=device), torch.full((6 * 17,), SENTINEL, dtype=torch.float32, device=device)
    fs, r0 = _dev_ints([6], torch.int32, device), _dev_ints([0], torch.int64, device)
    r, o, fp, rp = rows.data_ptr(), out.data_ptr(), fs.data_ptr(), r0.data_ptr()
    call = lib.disco_crnn_expand_rows
    assert call(None, None, 6, 1, 6, 17, fp, rp, o, None) == -1
    assert call(None, r, 6, 1, 6, 17, None, rp, o, None) == -1
    assert call(None, r, 6, 1, 6, 17, fp, None, o, None) == -1
    assert call(None, r, 6, 1, 6, 17, fp, rp, None, None) == -1
    assert call(None, r, 0, 1, 6, 17, fp, rp, o, None) == -1
    assert call(None, r, 6, 0, 6, 17, fp, rp, o, None) == -1
    assert call(None, r, 6, 1, 0, 17, fp, rp, o, None) == -1
    assert call(None, r, 6, 1, 6, 0, fp, rp, o, None) == -1
    pc._sync(out)
    assert bool((out == SENTINEL).all()), 'a refused call wrote to its output'
    return True


def check_beyond_one_grid_pass(lib, device, B=300, T=300, F=257, C=64, n_keep=2048, seed=5):
    """B = 300 signals of up to 300 frames (seeded in [2, 300]): more items than one pass of the capped launch grids covers, for the
    feature map (against the rectangular entry), the window gather and the placement of the output rows (against the same rows by torch
    indexing).  GPU only (hundreds of megabytes)."""
    import torch
    rng = np.random.default_rng(seed)
    frames_sig = rng.integers(2, T + 1, B)
    frames_sig[0], frames_sig[-1] = T, 2
    N, row0 = int(frames_sig.sum()), _row0(frames_sig)
    g = torch.Generator(device=device).manual_seed(seed)
    fd, r0 = _dev_ints(frames_sig, torch.int32, device), _dev_ints(row0, torch.int64, device)
    b_idx = torch.from_numpy(np.repeat(np.arange(B), frames_sig)).to(device)
    t_idx = torch.from_numpy(np.concatenate([np.arange(n) for n in frames_sig])).to(device)
    # the feature map: 8 rooms x 4 nodes, 4 channels of 320 rows of 257 = 10.5 M floats, bit for bit the rectangular entry's in the frames that exist
    from disco_amd.dnn.crnn import STFT_MAX, STFT_MIN
    Rf, Kf, Mf = 8, 4, 2
    fr_room = frames_sig[:Rf].copy()
    X = torch.view_as_complex(torch.randn((Rf, Kf, T, F, Mf, 2), device=device, generator=g))
    z = torch.view_as_complex(torch.randn((Rf, Kf, T, F, 2), device=device, generator=g))
    for r, Tr in enumerate(fr_room):
        X[r, :, Tr:], z[r, :, Tr:] = float('nan'), float('inf')
    frd = _dev_ints(fr_room, torch.int32, device)
    rect = torch.empty((Rf, Kf, Kf, T + 20, F), dtype=torch.float32, device=device)
    feat = torch.full_like(rect, SENTINEL)
    assert lib.disco_crnn_features(None, X.data_ptr(), z.data_ptr(), Rf, Kf, Mf, T, F, 1, 10, 10, STFT_MIN, STFT_MAX, rect.data_ptr(), pc._stream(X)) == 0
    assert lib.disco_crnn_features_rooms(None, X.data_ptr(), z.data_ptr(), Rf, Kf, Mf, T, F, 1, 10, 10, STFT_MIN, STFT_MAX, frd.data_ptr(),
                                         feat.data_ptr(), pc._stream(X)) == 0
    assert rect.numel() > (1 << 14) * 256
    for r, Tr in enumerate(fr_room):
        rect[r, :, :, 10 + int(Tr):] = 0.0
    assert torch.equal(feat.view(torch.int32), rect.view(torch.int32))
    del X, z, rect, feat
    # the output rows
    rows = torch.randn((N, F), device=device, generator=g)
    out = torch.full((B, T, F), SENTINEL, dtype=torch.float32, device=device)
    assert lib.disco_crnn_expand_rows(None, rows.data_ptr(), N, B, T, F, fd.data_ptr(), r0.data_ptr(), out.data_ptr(), pc._stream(rows)) == 0
    want = torch.zeros((B, T, F), device=device)
    want[b_idx, t_idx] = rows
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    del out, want, rows
    # the windows
    Tp = T + W - 1
    feat = torch.randn((B, C, Tp, FY), device=device, generator=g)
    got = torch.full((N + 1, n_keep), SENTINEL, dtype=torch.float32, device=device)
    assert lib.disco_crnn_windows_rooms(None, feat.data_ptr(), B, C, Tp, T, W, n_keep, fd.data_ptr(), r0.data_ptr(), got.data_ptr(), N,
                                        pc._stream(feat)) == 0
    c_used = -(-n_keep // (W * FY))
    win = feat.as_strided((B, T, c_used, W * FY), (feat.stride(0), FY, feat.stride(1), 1))
    assert bool((got[N] == SENTINEL).all())
    for lo in range(0, N, 8192):                                    # (in slices: the index gather makes a copy of what it reads)
        hi = min(N, lo + 8192)
        ref = win[b_idx[lo:hi], t_idx[lo:hi]].reshape(hi - lo, -1)[:, :n_keep]
        assert torch.equal(got[lo:hi], ref), lo
    return N / (B * T)


# ---- CRNN.predict_masks(..., frames=...) ---------------------------------------------------------------------------------------------
def _ragged_batch(n_ch, T, frames, device, dtype, seed, fill=float('nan')):
    import torch
    g = torch.Generator().manual_seed(seed)
    B = len(frames)
    level = torch.exp(2.0 * torch.randn((B, n_ch, T, 1), generator=g, dtype=torch.float64))      # loud and near-silent frames
    mag = torch.randn((B, n_ch, T, 257), generator=g, dtype=torch.float64).abs() * level
    for b, Tb in enumerate(frames):
        mag[b, :, Tb:] = fill                                       # what the batch holds beyond an item's frames is never seen
    return mag.to(device=device, dtype=dtype)


def check_predict_masks_frames(device, n_ch, frame_to_pred, dtype, tol, T=40, frames=(40, 2, 23), fused=True, seed=3, out_gain=40.0, alone_tol=0.0):
    """predict_masks(mag, frames=...)[b, :T_b] against predict_masks_windowed(mag[b, :, :T_b]) in float64 -- the reference's own evaluation
    order on the truncated sequence, no new code in it -- exact zeros beyond T_b, several groupings of the rows, and the `prepared` form."""
    import copy
    import torch
    from disco_amd.dnn.crnn import STFT_MAX, STFT_MIN, frames_to_pad
    model = rand_model(n_ch, seed, device, out_gain).to(dtype)
    model.fused_first_block = fused
    ref_model = copy.deepcopy(model).double()
    mag = _ragged_batch(n_ch, T, frames, device, dtype, seed)
    want = [ref_model.predict_masks_windowed(mag[b, :, :Tb].double(), frame_to_pred) for b, Tb in enumerate(frames)]
    worst = worst_alone = 0.0
    pad = frames_to_pad(frame_to_pred, model.x_out)
    prep = torch.nn.functional.pad(torch.clamp(mag, STFT_MIN, STFT_MAX), (0, 0, pad[0], pad[1]))
    for b, Tb in enumerate(frames):
        prep[b, :, pad[0] + Tb:] = 0.0
    runs = [model.predict_masks(mag, frame_to_pred=frame_to_pred, frames=frames),
            model.predict_masks(mag, frame_to_pred=frame_to_pred, frames=np.asarray(frames, np.int32), chunk=1),       # groups of <= T rows
            model.predict_masks(mag, frame_to_pred=frame_to_pred, frames=torch.tensor(frames), chunk=2),
            model.predict_masks(prep, frame_to_pred=frame_to_pred, frames=frames, prepared=True)]
    # the item alone through the rectangular path in the SAME precision (with float32 and the x 40 output weights this needs no float64 bar)
    alone = [model.predict_masks(mag[b:b + 1, :, :Tb].contiguous(), frame_to_pred=frame_to_pred)[0] for b, Tb in enumerate(frames)]
    for got in runs:
        assert got.shape == (len(frames), T, 257) and got.dtype == dtype and got.device == mag.device
        for b, Tb in enumerate(frames):
            e = float((got[b, :Tb] - alone[b]).abs().max())
            worst_alone = max(worst_alone, e)
            assert e < (alone_tol or tol), ('against the item alone', b, Tb, e)
        for b, Tb in enumerate(frames):
            assert not _bits(got[b, Tb:].float()).any(), ('not +0.0 beyond T_b', b)
            e = float((got[b, :Tb].double() - want[b]).abs().max())
            worst = max(worst, e)
            assert e < tol, (b, Tb, e)
    return worst, worst_alone


def check_predict_masks_uniform_and_refusals(device, dtype, tol, n_ch=3, T=24, out_gain=40.0):
    """frames=None is the path as it was (here: against the windowed evaluation, and against frames = T for every item); frames together
    with a norm_type, a wrong count or a value beyond T is refused."""
    import pytest
    import torch
    import copy
    model = rand_model(n_ch, 4, device, out_gain).to(dtype)
    ref_model = copy.deepcopy(model).double()
    mag = _ragged_batch(n_ch, T, (T, T), device, dtype, 9)
    a = model.predict_masks(mag)
    b = model.predict_masks(mag, frames=(T, T))
    # frames=None is the rectangular path itself: the same bits with the keyword spelled out, and whatever the chunking of an earlier ragged call
    assert torch.equal(a, model.predict_masks(mag, frames=None)) and torch.equal(a, model.predict_masks(mag))
    for i in range(2):
        assert float((a[i].double() - ref_model.predict_masks_windowed(mag[i].double())).abs().max()) < tol
    assert float((a - b).abs().max()) < tol
    for nt in ('scale_to_unit_norm', 'scale_to_1', 'center_and_scale'):
        with pytest.raises(ValueError, match='norm_type'):
            model.predict_masks(mag, frames=(T, T - 1), norm_type=nt)
    for bad in ((T,), (T, T + 1), (T, -1), (T, T, T)):
        with pytest.raises(ValueError, match='frames'):
            model.predict_masks(mag, frames=bad)
    assert not model.predict_masks(mag, frames=(0, 0)).any()
    return True


# ---- the two routes (GPU) ------------------------------------------------------------------------------------------------------------
def _oracle_with_masks(room, mz, mw, L):
    """float64 oracle of one room alone at its own length, fed masks (K, T_r, F) -> (oracle dict, time outputs per node)"""
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    y, s, n = room
    K = y.shape[0]
    masks = ([mz[k].T.astype(np.float64) for k in range(K)], [mw[k].T.astype(np.float64) for k in range(K)])
    o = to.offline_tango_vec(y, s, n, masks=masks, precision='f64', solver='eigh')
    return o, [so.istft(o['yf'][k], L, work_dtype=np.float64) for k in range(K)]


def _network_on_oracle_spectra(o, K, cpu_z, cpu_w):
    """the float64 networks on the oracle's own |Y| and |z| (tests/test_gpu_crnn_inloop.py) -> masks (K, T_r, F) of step 1, of step 2 or None"""
    import torch
    mag = np.stack([np.abs(o['Y'][k][0]).T for k in range(K)])[:, None]
    ref_mz = cpu_z.predict_masks(torch.from_numpy(mag)).numpy()
    if cpu_w is None:
        return ref_mz, None
    zmag = [np.abs(o['z_y'][j]).T for j in range(K)]
    inp = np.stack([np.stack([np.abs(o['Y'][k][0]).T] + [zmag[j] for j in range(K) if j != k]) for k in range(K)])
    return ref_mz, cpu_w.predict_masks(torch.from_numpy(inp)).numpy()


def check_in_loop(lib, K, M, two_models, lengths=LENGTHS, alone_only=False):
    """tango_enhance_dnn on a mixed batch whose padding holds NaN.  Per room: against the float64 oracle of that room alone at L_r fed the
    returned masks cropped to T_r; the masks against the float64 networks on the oracle's spectra; zeros beyond T_r / L_r; and against the
    same room on a uniform engine of its own length.  alone_only: just the uniform runs against the oracle (how the lengths were vetted).
    Every room is scored."""
    import torch
    import length_checks as lc
    from disco_amd.dnn.inloop import tango_enhance_dnn
    from disco_amd.engine import Engine
    R, Lmax, H = len(lengths), max(lengths), 256
    dev = torch.device('cuda', 0)
    model_z = rand_model(1, 1, dev)
    model_w = rand_model(K, 2, dev) if (two_models and K > 1) else None
    cpu_z = rand_model(1, 1, 'cpu').double()
    cpu_w = rand_model(K, 2, 'cpu').double() if model_w is not None else None
    y, s, n, own = lc.mixed_rooms(K, M, lengths, Lmax)
    errs = {}

    def worst(key, v):
        errs[key] = max(errs.get(key, 0.0), float(v))

    def score(tag, room, L, out, mz, mw):
        o, t_ref = _oracle_with_masks(room, mz, mw, L)
        for k in range(K):
            worst(tag + 'out', pc.relerr(out[k], t_ref[k]))
        ref_mz, ref_mw = _network_on_oracle_spectra(o, K, cpu_z, cpu_w)
        worst(tag + 'mask_z', np.abs(ref_mz - mz).max())
        if ref_mw is not None:
            worst(tag + 'mask_w', np.abs(ref_mw - mw).max())

    solo = []
    for r, L in enumerate(lengths):
        e1 = Engine(rooms=1, nodes=K, mics=M, length=int(L), lib=lib)
        res = tango_enhance_dnn(e1, torch.from_numpy(own[r][0][None]).to(dev), model_z, model_w, want_masks=True)
        solo.append([a.cpu().numpy()[0] for a in res])
        if alone_only:
            score('alone_', own[r], L, *solo[-1])
    if alone_only:
        print('each room alone on the uniform path', (K, M, two_models), errs)
        return errs

    eng = Engine(rooms=R, nodes=K, mics=M, length=Lmax, lib=lib)
    eng.set_lengths(lengths)
    assert np.isnan(y[np.argmin(lengths), 0, 0, -1])
    out, mz, mw = (a.cpu().numpy() for a in tango_enhance_dnn(eng, torch.from_numpy(y).to(dev), model_z, model_w, want_masks=True))
    assert np.isfinite(out).all() and np.isfinite(mz).all() and np.isfinite(mw).all(), 'the NaN beyond L_r surfaced'
    assert np.all((mz >= 0) & (mz <= 1)) and np.all((mw >= 0) & (mw <= 1))
    for r, L in enumerate(lengths):
        assert lc.scorable(L, 512) and L >= 16000
        Tr = 1 + L // H
        assert not mz[r, :, Tr:].any() and not mw[r, :, Tr:].any(), ('masks beyond T_r', r)
        assert not out[r, :, L:].any(), ('samples beyond L_r', r)
        score('', own[r], L, out[r, :, :L], mz[r, :, :Tr], mw[r, :, :Tr])
        worst('vs_alone_mask_z', np.abs(mz[r, :, :Tr] - solo[r][1]).max())
        worst('vs_alone_mask_w', np.abs(mw[r, :, :Tr] - solo[r][2]).max())
        if model_w is None:
            assert np.array_equal(mw[r], mz[r])                      # tango.py:388-389
    print('mixed lengths, CRNN masks in the loop', (K, M, two_models), errs)
    assert errs['out'] < CRNN_TOL and errs['mask_z'] < MASK1_TOL and errs.get('mask_w', 0.0) < MASK2_TOL, errs
    assert errs['vs_alone_mask_z'] < ALONE_TOL and errs['vs_alone_mask_w'] < ALONE_TOL, errs
    # given masks keep working with lengths set, and give the same samples
    again = tango_enhance_dnn(eng, torch.from_numpy(y).to(dev), None, None, masks=(torch.from_numpy(mz).to(dev), torch.from_numpy(mw).to(dev)))
    assert np.array_equal(again.cpu().numpy(), out)
    # without lengths not one call changes: the same engine, lengths taken back, against a fresh uniform engine
    eng.set_lengths(None)
    yu = np.nan_to_num(y)
    a = tango_enhance_dnn(eng, torch.from_numpy(yu).to(dev), model_z, model_w, want_masks=True)
    b = tango_enhance_dnn(Engine(rooms=R, nodes=K, mics=M, length=Lmax, lib=lib), torch.from_numpy(yu).to(dev), model_z, model_w, want_masks=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    return errs


NAMES = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']
SURFACE_VARIANTS = {'crnn2': (['crnn', 'crnn'], (True, True)), 'crnn1': (['crnn', 'crnn'], (True, False)),
                    'crnn_irm': (['crnn', 'irm1'], (True, False)), 'irm_crnn': (['irm1', 'crnn'], (False, True))}


def check_surface(device, variant, lengths=LENGTHS, K=3, M=2, oracle=True):
    """offline_tango_rooms with 'crnn' in vads and models in `mods`: per room the reference's 9-tuple of (257, T_r) arrays.  With 'crnn' at
    both steps: the seven spectra against the float64 oracle of the room alone fed the returned masks, and against offline_tango on the
    room alone (CRNN_TOL both).  Every predicted mask against offline_tango on the room alone
    (ALONE_TOL).  The engine cache is left without lengths."""
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango, offline_tango_batched, offline_tango_rooms
    from oracle import tango_oracle as to
    rooms = [synth.make_room_numpy(r, K=K, M=M, L=int(L))[:3] for r, L in enumerate(lengths)]
    vads, use = SURFACE_VARIANTS[variant]
    mods = [rand_model(1, 1, device) if use[0] else None, rand_model(K, 2, device) if use[1] else None]
    errs = {}

    def worst(key, v):
        errs[key] = max(errs.get(key, 0.0), float(v))

    res = offline_tango_rooms([tuple(list(a) for a in room) for room in rooms], vads=vads, mods=mods)
    assert len(res) == len(rooms)
    for r, (L, room) in enumerate(zip(lengths, rooms)):
        Tr = 1 + L // 256
        assert len(res[r]) == 9 and all(a.shape == (257, Tr) and np.isfinite(a).all() for part in res[r] for a in part), (variant, r)
        sep = offline_tango(list(room[0]), list(room[1]), list(room[2]), vads=vads, mods=mods)
        for k in range(K):
            for i, v in ((7, vads[0]), (8, vads[1])):
                if v == 'crnn':
                    worst(NAMES[i] + '_vs_alone', np.abs(res[r][i][k] - sep[i][k]).max())
            if vads == ['crnn', 'crnn']:
                for i in range(7):
                    worst('spectra_vs_alone', pc.relerr(res[r][i][k], sep[i][k]))
        if oracle and vads == ['crnn', 'crnn']:
            o = to.offline_tango_vec(*room, masks=([m.astype(np.float64) for m in res[r][7]], [m.astype(np.float64) for m in res[r][8]]),
                                     precision='f64', solver='eigh')
            ref = to.as_reference_tuple(o)
            for i in range(7):
                for k in range(K):
                    worst('spectra_vs_oracle', pc.relerr(res[r][i][k], ref[i][k]))
        if variant == 'crnn1':
            assert all(np.array_equal(res[r][8][k], res[r][7][k]) for k in range(K))       # tango.py:388-389
    print('offline_tango_rooms, CRNN masks', variant, errs)
    assert errs.get('spectra_vs_oracle', 0.0) < CRNN_TOL and errs.get('spectra_vs_alone', 0.0) < CRNN_TOL, errs
    assert errs.get('masks_z_vs_alone', 0.0) < ALONE_TOL and errs.get('mask_w_vs_alone', 0.0) < ALONE_TOL, errs
    # the cached engines are left without lengths
    Ls = min(lengths)
    d = offline_tango_batched(*(np.stack([a[..., :Ls] for a in room3]) for room3 in zip(*rooms)), vads=vads, mods=mods)
    assert d['yf'][0, :, -1].any() and d['masks_z'][0, :, -1].any()
    return errs
