"""Why a batch needs per-room lengths (disco_set_lengths), pinned with the float64 oracle alone -- no library involved: zero-padding a
clip to the longest of its batch is NOT the computation the reference does on the clip itself.  The reference reflects each clip at its
own end (librosa.stft(center=True)), averages the covariances over its own T = 1 + L / hop frames, and istft(length=L) normalises the
last half window by the window sum of its own frame count."""
import numpy as np

import length_checks as lc
from disco_amd import synth
from oracle import stft_oracle as so
from oracle import tango_oracle as to

N_FFT, HOP = 512, 256


def _enhanced(y, s, n):
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    L = y.shape[-1]
    return [so.istft(o['yf'][k], L, N_FFT, HOP, work_dtype=np.float64) for k in range(y.shape[0])]


def test_zero_padding_a_clip_is_another_computation():
    """rooms 1-5 of the (3, 2) test shape padded with zeros to the 12288 samples of room 0: the valid part of every node's enhanced signal
    moves by more than 1e-3 relative, ten times the project's bar of 1e-4 (measured: 6.7e-2 ... 5.1e-1)"""
    K, M, Lmax = 3, 2, lc.LENGTHS_K3M2[0]
    moved = {}
    for r, L in list(enumerate(lc.LENGTHS_K3M2))[1:]:
        y, s, n = synth.make_room_numpy(r, K=K, M=M, L=L)[:3]
        own = _enhanced(y, s, n)
        pad = [np.concatenate([a, np.zeros(a.shape[:-1] + (Lmax - L,), a.dtype)], axis=-1) for a in (y, s, n)]
        padded = _enhanced(*pad)
        moved[L] = [lc.relerr(padded[k][:L], own[k]) for k in range(K)]
        assert min(moved[L]) > 1e-3, (L, moved[L])
    print(moved)


def test_window_sum_of_the_last_segment_follows_the_clip():
    """a spectrum whose frames beyond T_r are zero, inverted at the batch's length, equals the clip's own inverse transform except in the
    last L_r % hop samples: there the clip's own transform divides by the window sum of T_r frames (the last frame alone)"""
    rng = np.random.default_rng(0)
    Lmax, F = 12288, N_FFT // 2 + 1
    Tmax = 1 + Lmax // HOP
    for L in (8193, 10000, 6272, 11100, 6143):
        Tr, tail = 1 + L // HOP, L % HOP
        Z = np.zeros((F, Tmax), np.complex128)
        Z[:, :Tr] = rng.standard_normal((F, Tr)) + 1j * rng.standard_normal((F, Tr))
        rect = so.istft(Z, Lmax, N_FFT, HOP, work_dtype=np.float64)[:L]
        own = so.istft(Z[:, :Tr], L, N_FFT, HOP, work_dtype=np.float64)
        assert np.allclose(rect[:L - tail], own[:L - tail], rtol=1e-12, atol=1e-12)
        # ... exactly by the ratio of the two window sums, which grows from 1 at the segment's first sample (the window starts at 0)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
        w0, w1 = w[HOP:HOP + tail] ** 2, w[:tail] ** 2
        assert np.allclose(own[L - tail:] * w0, rect[L - tail:] * (w0 + w1), rtol=1e-9, atol=1e-12), L
        if tail >= 64:
            assert np.abs(own[L - tail:] - rect[L - tail:]).max() > 1e-2 * np.abs(own[L - tail:]).max(), L
    # a whole number of hops: nothing to differ in
    L = 5120
    Tr = 1 + L // HOP
    Z = np.zeros((F, Tmax), np.complex128)
    Z[:, :Tr] = rng.standard_normal((F, Tr)) + 1j * rng.standard_normal((F, Tr))
    assert np.allclose(so.istft(Z, Lmax, N_FFT, HOP, work_dtype=np.float64)[:L], so.istft(Z[:, :Tr], L, N_FFT, HOP, work_dtype=np.float64),
                       rtol=1e-12, atol=1e-12)
