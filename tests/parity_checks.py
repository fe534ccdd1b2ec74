"""Stage-by-stage and end-to-end comparisons of the HIP path (through the C ABI) with the CPU oracle.

Shared by tests/test_gpu_parity.py (real MI355X, `-m gpu`) and tests/test_kernels_emulated.py (the same
kernel sources under the hipemu CPU emulator, toy sizes, `-m "not gpu"`).  `make_engine(**cfg)` builds a
disco_amd.engine.Engine bound to the library under test.
"""
import numpy as np

from oracle import mwf_oracle as mo
from oracle import stft_oracle as so
from oracle import tango_oracle as to


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def maxrel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check_stft(make_engine, n_sig=2, chans=3, L=3000, n_fft=512, pad_mode='reflect', seed=0, tol=2e-6):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_sig, chans, L)).astype(np.float32)
    eng = make_engine(rooms=n_sig, nodes=1, mics=chans, length=L, n_fft=n_fft, pad_mode=pad_mode)
    X = eng.stft(x).numpy()                                              # (n_sig, T, F, chans)
    ref = so.stft(x, n_fft, n_fft // 2, pad_mode, np.complex128)         # (n_sig, chans, F, T)
    ref = np.transpose(ref, (0, 3, 2, 1))
    assert X.shape == ref.shape
    e = maxrel(X, ref)
    assert e < tol, e
    return e


def check_istft(make_engine, n_sig=3, L=3000, n_fft=512, seed=1, tol=3e-6):
    rng = np.random.default_rng(seed)
    T, F = 1 + L // (n_fft // 2), n_fft // 2 + 1
    Z = (rng.standard_normal((n_sig, T, F)) + 1j * rng.standard_normal((n_sig, T, F))).astype(np.complex64)
    eng = make_engine(rooms=n_sig, nodes=1, mics=1, length=L, n_fft=n_fft)
    y = eng.istft(Z).numpy()
    ref = so.istft(np.transpose(Z, (0, 2, 1)), L, n_fft, n_fft // 2, work_dtype=np.float64)
    e = maxrel(y, ref)
    assert e < tol, e
    # round trip on a real signal
    x = rng.standard_normal((n_sig, 1, L)).astype(np.float32)
    xr = eng.istft(eng.stft(x).reshape(n_sig, T, F)).numpy()
    e2 = float(np.abs(xr - x[:, 0]).max())
    assert e2 < 2e-5, e2
    return e


def check_masks(make_engine, L=3000, n_fft=512, seed=2):
    rng = np.random.default_rng(seed)
    n_sig = 2
    s = rng.standard_normal((n_sig, L)).astype(np.float32)
    n = rng.standard_normal((n_sig, L)).astype(np.float32)
    s[:, :400] = 0
    worst = 0.0
    for mask in ('irm1', 'irm2', 'iam1', 'ibm1'):
        eng = make_engine(rooms=n_sig, nodes=1, mics=1, length=L, n_fft=n_fft, mask=mask)
        m = eng.mask_oracle(s, n).numpy()                                # (n_sig, T, F)
        S = so.stft(s, n_fft, n_fft // 2, 'reflect', np.complex128)
        Nn = so.stft(n, n_fft, n_fft // 2, 'reflect', np.complex128)
        with np.errstate(all='ignore'):
            ref = np.transpose(mo.tf_mask(S, Nn, type=mask), (0, 2, 1)).astype(np.float64)
        if mask.startswith('ibm'):
            assert np.mean(m != ref) < 1e-3                              # threshold flips at rounding level only
        else:
            ok = np.isfinite(ref)
            err = np.abs(m[ok] - ref[ok]) / (1.0 + np.abs(ref[ok]))
            # the mask is a ratio of STFT magnitudes: where a denominator (|N|, or |S+N| for 'iam') nearly cancels
            # against the frame norm, fp32 STFT rounding is amplified -- bound the bulk tightly, the tail loosely
            e = float(np.percentile(err, 99.9))
            worst = max(worst, e)
            assert e < 2e-5 and float(err.max()) < 5e-3, (mask, e, float(err.max()))
        # elementwise entry point on given STFT planes
        S32, N32 = S.astype(np.complex64), Nn.astype(np.complex64)
        m2 = eng.tf_mask(S32, N32, type=mask).numpy()
        with np.errstate(all='ignore'):
            ref2 = mo.tf_mask(S32, N32, type=mask)
        if mask.startswith('ibm'):
            assert np.mean(m2 != ref2) < 1e-3
            above = np.abs(S32) >= mo.EPS                                # exact ties |S| = |N| above the clamp: the reference divides and answers 1
            for tie in (S32, -S32, np.conj(S32)):
                assert mo.tf_mask(S32, tie, type=mask)[above].all() and eng.tf_mask(S32, tie, type=mask).numpy()[above].all()
        else:
            ok = np.isfinite(ref2)
            assert float((np.abs(m2[ok] - ref2[ok]) / (1.0 + np.abs(ref2[ok]))).max()) < 1e-5
    return worst


def _rand_stft_scene(rng, R, K, M, T, F):
    """Spatially structured random STFTs (rank-1 target + full-rank noise per bin) and a mask in (0,1)."""
    a = rng.standard_normal((R, K, 1, F, M)) + 1j * rng.standard_normal((R, K, 1, F, M))
    src = rng.standard_normal((R, 1, T, F, 1)) + 1j * rng.standard_normal((R, 1, T, F, 1))
    noise = rng.standard_normal((R, K, T, F, M)) + 1j * rng.standard_normal((R, K, T, F, M))
    X = (a * src + 0.7 * noise).astype(np.complex64)
    mask = rng.uniform(0.05, 0.95, (R, K, T, F)).astype(np.float32)
    return X, mask


def oracle_cov(X, mask, Zs=None, Zn=None, mask_remote=True):
    """float64 restatement of tango.py:357-364 / 433-440 in the engine's layout."""
    R, K, T, F, M = X.shape
    X = X.astype(np.complex128)
    m = mask.astype(np.float64)[..., None]
    P = M + (K - 1 if Zs is not None else 0)
    Rss = np.zeros((R, K, F, P, P), np.complex128)
    Rnn = np.zeros_like(Rss)
    for k in range(K):
        vs = [m[:, k] * X[:, k]]
        vn = [(1 - m[:, k]) * X[:, k]]
        if Zs is not None and K > 1:
            others = [j for j in range(K) if j != k]
            gs = m[:, k] if mask_remote else 1.0
            gn = (1 - m[:, k]) if mask_remote else 1.0
            vs.append(gs * np.stack([Zs[:, j].astype(np.complex128) for j in others], axis=-1))
            vn.append(gn * np.stack([Zn[:, j].astype(np.complex128) for j in others], axis=-1))
        vs = np.concatenate(vs, axis=-1)
        vn = np.concatenate(vn, axis=-1)
        Rss[:, k] = np.einsum('rtfp,rtfq->rfpq', vs, vs.conj()) / T
        Rnn[:, k] = np.einsum('rtfp,rtfq->rfpq', vn, vn.conj()) / T
    return Rss, Rnn


def check_cov_solve_apply(make_engine, R=2, K=2, M=2, L=2560, n_fft=512, seed=3, same_z=True, mask_remote=True, options=None):
    """options: {key: value} of disco_set_option for this context (e.g. {'solve_thread': 0}: the LDS group solver for 5 <= P <= 8)."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    for k_, v_ in (options or {}).items():
        eng.set_option(k_, v_)
        assert eng.get_option(k_) == v_
    T, F = eng.T, eng.F
    X, mask = _rand_stft_scene(rng, R, K, M, T, F)
    errs = {}
    # step-1 shape (P = M)
    Rss, Rnn = eng.cov_masked(X, mask)
    rs, rn = oracle_cov(X, mask)
    errs['cov1'] = max(relerr(Rss.numpy(), rs), relerr(Rnn.numpy(), rn))
    assert errs['cov1'] < 5e-6, errs
    wp, t1p = eng.gevd_mwf_r1_pending(M, want_t1=True)      # straight from the partial sums of the call above
    w, t1 = eng.gevd_mwf_r1(Rss, Rnn)
    w_ref, t1_ref, _ = mo.gevd_mwf_r1_hermitian(Rss.numpy(), Rnn.numpy(), 1.0)
    errs['solve1'] = max(relerr(w.numpy(), w_ref), relerr(t1.numpy(), t1_ref))
    # the pending solve works on the partial sums themselves (combined in float64, unscaled), `w_ref` on the complex64 means: two roundings
    # of the same sums.  For M >= 7 -- ill-conditioned 7 x 7 / 8 x 8 pencils move by 5e-6 under either rounding -- it is held to whichever of
    # the complex64 solution and the float64 oracle's is closer; every smaller shape to the complex64 solution alone (round-4 ADVICE).
    e_ref = max(relerr(wp.numpy(), w_ref), relerr(t1p.numpy(), t1_ref))
    if M >= 7:
        w_true, t1_true, _ = mo.gevd_mwf_r1_hermitian(rs, rn, 1.0)
        e_ref = min(e_ref, max(relerr(wp.numpy(), w_true), relerr(t1p.numpy(), t1_true)))
    errs['solve1_pending'] = e_ref
    assert errs['solve1'] < 5e-6 and errs['solve1_pending'] < 5e-6, errs
    z = eng.apply(X, w)
    z_ref = np.einsum('rkfm,rktfm->rktf', w.numpy().conj().astype(np.complex128), X.astype(np.complex128))
    errs['apply1'] = relerr(z.numpy(), z_ref)
    assert errs['apply1'] < 5e-6, errs
    zt = eng.apply(X, t1, conj=False).numpy()
    errs['apply1_t'] = relerr(zt, np.einsum('rkfm,rktfm->rktf', t1.numpy().astype(np.complex128), X.astype(np.complex128)))
    assert errs['apply1_t'] < 5e-6, errs
    zn = eng.noise_residual(X, z).numpy()
    assert relerr(zn, X[..., 0] - z.numpy()) < 1e-6
    if K > 1:
        zs = z.numpy()
        zn_arr = zs if same_z else (zs * 0.5 + 0.1 * X[..., 0]).astype(np.complex64)
        Rss2, Rnn2 = eng.cov_masked(X, mask, zs, zs if same_z else zn_arr, mask_remote=mask_remote)
        rs2, rn2 = oracle_cov(X, mask, zs, zn_arr, mask_remote)
        errs['cov2'] = max(relerr(Rss2.numpy(), rs2), relerr(Rnn2.numpy(), rn2))
        assert errs['cov2'] < 5e-6, errs
        w2, t12 = eng.gevd_mwf_r1(Rss2, Rnn2)
        w2_ref, _, _ = mo.gevd_mwf_r1_hermitian(Rss2.numpy(), Rnn2.numpy(), 1.0)
        errs['solve2'] = relerr(w2.numpy(), w2_ref)
        assert errs['solve2'] < 5e-6, errs
        yf = eng.apply(X, w2, Z=zs).numpy()
        ext = []
        for k in range(K):
            others = [j for j in range(K) if j != k]
            ext.append(np.concatenate([X[:, k].astype(np.complex128)] + [zs[:, j, :, :, None].astype(np.complex128) for j in others], axis=-1))
        ext = np.stack(ext, axis=1)                                       # (R,K,T,F,P)
        yf_ref = np.einsum('rkfp,rktfp->rktf', w2.numpy().conj().astype(np.complex128), ext)
        errs['apply2'] = relerr(yf, yf_ref)
        assert errs['apply2'] < 5e-6, errs
    return errs


def check_stft_cov_fused(make_engine, R=2, K=2, M=4, L=30000, n_fft=512, seed=6, tuning=None):
    """STFT + step-1 covariance in one pass vs the two staged kernels it replaces (1024-point STFT with 7 or 8 microphones: the
    entry point itself runs the two passes)."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((R, K, M, L)).astype(np.float32)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    if tuning is not None:
        eng.set_tuning(*tuning)
    mask = rng.uniform(0.05, 0.95, (R, K, eng.T, eng.F)).astype(np.float32)
    X, Rss, Rnn = eng.stft_cov_fused(y, mask)
    Xs = eng.stft(y.reshape(R * K, M, L)).reshape(R, K, eng.T, eng.F, M)
    # same algorithm; hipcc may contract mul+add into fma differently in the two kernels, so not bit-for-bit
    assert maxrel(X.numpy(), Xs.numpy()) < 1e-6
    rs, rn = oracle_cov(Xs.numpy(), mask)
    e = max(relerr(Rss.numpy(), rs), relerr(Rnn.numpy(), rn))
    assert e < 5e-6, e
    Rss_s, Rnn_s = eng.cov_masked(Xs, mask)
    e2 = max(relerr(Rss.numpy(), Rss_s.numpy()), relerr(Rnn.numpy(), Rnn_s.numpy()))
    assert e2 < 5e-6, e2
    return e, e2


def check_step2_fused(make_engine, R=2, K=4, M=4, L=4096, n_fft=512, seed=5):
    """The in-register z exchange kernels against the staged kernels they replace (same inputs -> same sums up to
    accumulation order) and against the float64 restatement."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    T, F = eng.T, eng.F
    X, mask = _rand_stft_scene(rng, R, K, M, T, F)
    P = M + K - 1
    w_loc = (rng.standard_normal((R, K, F, M)) + 1j * rng.standard_normal((R, K, F, M))).astype(np.complex64) * 0.3
    w_glo = (rng.standard_normal((R, K, F, P)) + 1j * rng.standard_normal((R, K, F, P))).astype(np.complex64) * 0.3
    z_ref = np.einsum('rkfm,rktfm->rktf', w_loc.conj().astype(np.complex128), X.astype(np.complex128))
    Rss, Rnn, z = eng.step2_cov_fused(X, mask, w_loc, want_z=True)
    errs = {'z': relerr(z.numpy(), z_ref)}
    assert errs['z'] < 2e-6, errs
    rs, rn = oracle_cov(X, mask, z_ref, z_ref, True)
    errs['cov2'] = max(relerr(Rss.numpy(), rs), relerr(Rnn.numpy(), rn))
    assert errs['cov2'] < 5e-6, errs
    if K > 1:
        zs = eng.apply(X, w_loc)
        Rss_s, Rnn_s = eng.cov_masked(X, mask, zs, zs, mask_remote=True)
        errs['cov2_vs_staged'] = max(relerr(Rss.numpy(), Rss_s.numpy()), relerr(Rnn.numpy(), Rnn_s.numpy()))
        assert errs['cov2_vs_staged'] < 5e-6, errs
    yf, z2 = eng.step2_apply_fused(X, w_loc, w_glo, want_z=True)
    ext = []
    for k in range(K):
        others = [j for j in range(K) if j != k]
        ext.append(np.concatenate([X[:, k].astype(np.complex128)] + [z_ref[:, j, :, :, None] for j in others], axis=-1))
    ext = np.stack(ext, axis=1)
    yf_ref = np.einsum('rkfp,rktfp->rktf', w_glo.conj().astype(np.complex128), ext)
    errs['yf'] = relerr(yf.numpy(), yf_ref)
    errs['z2'] = relerr(z2.numpy(), z_ref)
    assert errs['yf'] < 2e-6 and errs['z2'] < 2e-6, errs
    if n_fft == 512 and K > 1:
        # filter + iSTFT in one kernel vs the two kernels it replaces
        t_fused = eng.step2_apply_istft_fused(X, w_loc, w_glo).numpy()
        t_staged = eng.istft(yf.reshape(R * K, T, F)).numpy().reshape(R, K, L)
        errs['apply_istft'] = maxrel(t_fused, t_staged)
        assert errs['apply_istft'] < 3e-6, errs
    return errs


def check_step2_reuse(make_engine, R=1, K=3, M=2, L=6000):
    """disco_step2_cov_fused_reuse (leading M x M block taken from the step-1 partial sums) gives the same step-2
    filters as the full step-2 covariance; its contract violations are refused."""
    import pytest
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    T, F = eng.T, eng.F
    mask = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F)    # stays on the device:
    P = M + K - 1                                       # the re-use is granted for THE arrays the step-1 sums were computed from
    X, _, _ = eng.stft_cov_fused(y, mask)
    w_loc, _ = eng.gevd_mwf_r1_pending(M)
    with pytest.raises(Exception):          # another mask array (even with equal contents) is not what step 1 saw
        eng.step2_cov_fused_reuse(X, mask.numpy(), w_loc)
    z = eng.step2_cov_fused_reuse(X, mask, w_loc, want_z=True)
    w_a, t_a = eng.gevd_mwf_r1_pending(P, want_t1=True)
    Rss, Rnn, z_b = eng.step2_cov_fused(X, mask, w_loc, want_z=True)
    w_b, t_b = eng.gevd_mwf_r1(Rss, Rnn, want_t1=True)
    errs = {'z': relerr(z.numpy(), z_b.numpy()), 'w': relerr(w_a.numpy(), w_b.numpy()), 't1': relerr(t_a.numpy(), t_b.numpy())}
    assert errs['z'] == 0.0 and errs['w'] < 2e-5 and errs['t1'] < 2e-5, errs
    with pytest.raises(Exception):          # scratch now holds step-2 sums: nothing to re-use
        eng.step2_cov_fused_reuse(X, mask, w_loc)
    return errs


def check_online_golden(make_engine, golden_dir, t_max=None):
    """disco_online_mwf against outputs of the reference's own spatial_correlation_matrix + intern_filter driven frame by
    frame (tests/golden/make_golden_online.py).  The recursion is causal, so a prefix of the golden frames is itself a
    golden case (t_max: the slow CPU emulation runs a prefix only)."""
    import os
    g = np.load(os.path.join(golden_dir, 'online_ref.npz'))
    errs = {}
    for tag in ('p3', 'p5u4'):
        V, mask, ref, w_ref = g[tag + '_V'], g[tag + '_mask'], g[tag + '_out'], g[tag + '_w']
        lam, mu, init, U = (float(x) for x in g[tag + '_params'])
        if t_max is not None:
            V, mask, ref, w_ref = V[:, :, :t_max], mask[:, :t_max], ref[:, :t_max], w_ref[:, :t_max]
        P, F, T = V.shape
        # one room, one node with P "mics"; the golden bins occupy the first F of the engine's 257, the rest carry zeros
        eng = make_engine(rooms=1, nodes=1, mics=P, length=(T - 1) * 256, n_fft=512)
        assert eng.T == T, (eng.T, T)
        X = np.zeros((1, 1, T, eng.F, P), np.complex64)
        X[0, 0, :, :F] = V.transpose(2, 1, 0)
        mk = np.full((1, 1, T, eng.F), 0.5, np.float32)
        mk[0, 0, :, :F] = mask.T
        out, w = eng.online_mwf(X, mk, lambda_cor=lam, mu=mu, update_every=int(U), init_diag=init, want_w=True)
        out, w = out.numpy()[:, :, :, :F], w.numpy()[:, :, :F]
        assert np.isfinite(out).all()
        errs[tag] = relerr(out[0, 0].T, ref)
        errs[tag + '_w'] = relerr(w[0, 0], w_ref[:, -1])
        assert errs[tag] < 5e-5 and errs[tag + '_w'] < 5e-5, errs
    return errs


def check_online_mwf(make_engine, R=2, K=3, M=2, L=6000, n_fft=512, update_every=1, tol=1e-4):
    """Both launches of the online kernel (P = M and P = M + K - 1 with the exchanged z) and the whole online pipeline
    against oracle/online_oracle.py on synthetic rooms."""
    from disco_amd import synth
    from oracle import online_oracle as oo
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    T, F = eng.T, eng.F
    mask = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F).numpy()
    out, z, yf = eng.tango_online(y, mask, update_every=update_every)
    out, z, yf = out.numpy(), z.numpy(), yf.numpy()
    errs = {'z': 0.0, 'yf': 0.0, 'out': 0.0}
    for r in range(R):
        o = oo.online_tango(y[r], s[r], n[r], n_fft=n_fft, hop=n_fft // 2, update_every=update_every)
        for k in range(K):
            errs['z'] = max(errs['z'], relerr(z[r, k].T, o['z'][k]))
            errs['yf'] = max(errs['yf'], relerr(yf[r, k].T, o['yf'][k]))
            errs['out'] = max(errs['out'], relerr(out[r, k], o['out'][k]))
    assert errs['z'] < tol and errs['yf'] < tol and errs['out'] < tol, errs
    # option "online_sq32" = 0: the thread solves (P <= 7) with float64 squarings; both routes within the bar, and close to each other
    e64 = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    e64.set_option('online_sq32', 0)
    out64 = e64.tango_online(y, mask, update_every=update_every)[0].numpy()
    errs['out_f64_squarings'] = max(relerr(out64[r, k], oo.online_tango(y[r], s[r], n[r], n_fft=n_fft, hop=n_fft // 2,
                                                                         update_every=update_every)['out'][k])
                                    for r in range(R) for k in range(K))
    errs['sq32_vs_f64'] = relerr(out, out64)
    assert errs['out_f64_squarings'] < tol and errs['sq32_vs_f64'] < 2e-5, errs
    # the staged call with a node shard: nodes [1, K) only, remote rows from the full z
    if K > 1:
        X = eng.stft(y.reshape(R * K, M, L)).numpy().reshape(R, K, T, F, M)
        sh = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        sh.set_node_shard(1, K - 1)
        yf_sh = sh.online_mwf(X[:, 1:], mask[:, 1:], Z=z, update_every=update_every).numpy()
        errs['sharded'] = relerr(yf_sh, yf[:, 1:])
        assert errs['sharded'] < 1e-6, errs
    return errs


def check_online_stream(make_engine, R=2, K=3, M=2, L=6144, n_fft=512, update_every=3, chunks=(2, 5, 1, 7, 3), options=None):
    """disco_tango_online_stream (state in, state out: the online path fed chunk by chunk) against disco_tango_online on the whole clip:
    the same output samples BIT FOR BIT, whatever the chunking -- ragged chunk sizes (cycled from `chunks`, in hops), a one-hop chunk,
    filter updates that fall inside chunks, the final frame delivered with the last chunk (last=True needs new samples: the stream is not
    flushed empty-handed) -- and the state block really carries everything
    (a second stream interleaved on the same context does not disturb the first; a copy of the block resumes a stream).
    options: {key: value} applied with set_option before the first call (solve_thread = 0: the group kernel at P <= 7)."""
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    H = n_fft // 2
    assert L % H == 0
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    for key, value in (options or {}).items():
        eng.set_option(key, value)
    T, F = eng.T, eng.F
    mask = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F).numpy()
    whole = eng.tango_online(y, mask, update_every=update_every, want_z=False, want_yf=False)[0].numpy()
    n_hops_total = L // H

    def run(sizes, interleave=None):
        st = eng.online_stream(update_every=update_every)
        other = eng.online_stream(update_every=update_every) if interleave else None
        got, h, i = [], 0, 0
        while h < n_hops_total:
            c = min(sizes[i % len(sizes)], n_hops_total - h)
            if h == 0:
                c = max(c, 2)
            i += 1
            last = h + c == n_hops_total
            got.append(st.push(y[..., h * H:(h + c) * H], mask[:, :, h:h + c + (1 if last else 0)], last=last))
            if other is not None and h == 0:            # another stream of the same context in between: must not matter
                other.push(0.5 * y[..., :c * H], mask[:, :, :c])
            h += c
        return np.concatenate(got, axis=-1)
    res = {}
    for name, sizes, inter in (('ragged', chunks, False), ('one_call', (n_hops_total,), False), ('interleaved', (4,), True), ('hop_by_hop', (1,), False)):
        out = run(sizes, inter)
        assert out.shape == whole.shape, (name, out.shape, whole.shape)
        res[name] = float(np.abs(out - whole).max())
        assert np.array_equal(out, whole), (name, res[name])
    return res


def check_metrics(make_engine, golden_dir, L_cut=None, start=0):
    """disco_amd.metrics (HIP moments + host dB arithmetic) against the reference's own metrics.py outputs
    (tests/golden/metrics_ref.npz) and against oracle/metrics_oracle.py on a sub-span (start > 0: the reference scores
    [fs:], tango.py:553).  L_cut: the slow CPU emulation runs a short span only (then only the oracle comparison applies)."""
    import os
    from disco_amd import metrics as gm
    from oracle import metrics_oracle as mo
    g = np.load(os.path.join(golden_dir, 'metrics_ref.npz'))
    fs = int(g['fs'])
    sig = {k: g[k] if L_cut is None else np.ascontiguousarray(g[k][:2, 3800:3800 + L_cut]) for k in ('s_in', 'n_in', 's_out', 'n_out', 'vad_tar', 'vad_noi')}
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    saved = gm._engine
    gm._engine = lambda: eng
    try:
        s_in, n_in, s_out, n_out = (sig[k] for k in ('s_in', 'n_in', 's_out', 'n_out'))
        C = s_in.shape[0]
        got = {'snr_in': gm.snr(s_in, n_in, start=start), 'delta_snr': gm.delta_snr(s_out, n_out, s_in, n_in, start=start),
               'sd': gm.sd(s_out, s_in, start=start), 'si_sdr': gm.si_sdr(s_in, s_out + n_out, start=start)}
        got['fw_snr'], got['fw_snr_mean'], F = gm.fw_snr(s_out, n_out, fs, start=start)
        # fw_snr(..., vad_tar, vad_noi) (metrics.py:63, 104-112), in the reference's argument positions
        got['fw_snr_vad'], got['fw_snr_vad_mean'], _ = gm.fw_snr(s_out, n_out, fs, sig['vad_tar'], sig['vad_noi'], start=start)
        got['fw_sd'], got['fw_sd_mean'], _ = gm.fw_sd(s_out, s_in, fs, start=start)
        got['si_bss'] = np.stack(gm.si_bss(s_out + n_out, [s_in, n_in], 0, start=start), axis=-1)
    finally:
        gm._engine = saved
    errs = {}
    for c in range(C):
        a, b, x, y = s_in[c, start:], n_in[c, start:], s_out[c, start:], n_out[c, start:]
        want = {'snr_in': mo.snr(a, b), 'delta_snr': mo.delta_snr(x, y, a, b), 'sd': mo.sd(x, a),
                'si_sdr': mo.si_sdr(a, (s_out + n_out)[c, start:]), 'fw_snr': mo.fw_snr(x, y, fs)[0],
                'fw_snr_mean': mo.fw_snr(x, y, fs)[1], 'fw_sd': mo.fw_sd(x, a, fs)[0], 'fw_sd_mean': mo.fw_sd(x, a, fs)[1],
                'si_bss': np.array(mo.si_bss((s_out + n_out)[c, start:].astype(np.float64),
                                             np.stack([a, b], 1).astype(np.float64), 0))}
        want['fw_snr_vad'], want['fw_snr_vad_mean'], _ = mo.fw_snr(x, y, fs, sig['vad_tar'][c, start:], sig['vad_noi'][c, start:])
        for k, v in want.items():
            assert np.all(np.isfinite(v)) and np.all(np.isfinite(np.asarray(got[k])[c])), (k, v, np.asarray(got[k])[c])
            errs[k] = max(errs.get(k, 0.0), float(np.max(np.abs(np.asarray(got[k])[c] - v))))
    assert all(e < 2e-4 for e in errs.values()), errs                 # dB; float32-vs-float64 variance of the reference
    if L_cut is None and start == 0:
        for k in got:
            e = float(np.max(np.abs(np.asarray(got[k]) - g[k])))
            errs[k + '_vs_reference'] = e
            assert e < 2e-4, (k, e)
        assert np.array_equal(F, g['F'])
    return errs


def check_ivad(make_engine, golden_dir):
    """disco_mask_ivad against the reference's own vad_oracle_batch / get_mask('ivad') outputs (tests/golden/ivad_ref.npz)."""
    import os
    g = np.load(os.path.join(golden_dir, 'ivad_ref.npz'))
    errs = {}
    for i in range(int(g['n_vad'])):
        x, vad = g[f'vad_x{i}'], g[f'vad_o{i}']
        L = len(x)
        eng = make_engine(rooms=1, nodes=1, mics=1, length=L)
        m = eng.mask_ivad(x[None]).numpy()[0]                       # (T, F)
        want = np.zeros(eng.T)
        v = vad[::256]
        want[:len(v)] = v
        assert np.all(m == m[:, :1]), 'mask must be constant over frequency'
        errs[f'vad{i}_frames_wrong'] = int(np.sum(m[:, 0] != want))
        assert errs[f'vad{i}_frames_wrong'] == 0, errs
    K, L = int(g['K']), int(g['L'])
    eng = make_engine(rooms=1, nodes=K, mics=2, length=L)
    for k in range(K):
        m = eng.mask_ivad(g[f's{k}'][0][None]).numpy()[0]
        errs[f'mask{k}_wrong'] = int(np.sum(m.T != g[f'masks_z{k}']))
        assert errs[f'mask{k}_wrong'] == 0, errs
    return errs


def check_rir_convolve(make_engine, n_sig=2, n_ch=3, Ld=3000, Lh=700, out_len=None, seed=3, tol=2e-6):
    """disco_rir_convolve == np.convolve(dry, rir)[:out_len] (the reference's own line, gen_disco/convolve_signals.py:160-163),
    float64 on the host side of the comparison."""
    rng = np.random.default_rng(seed)
    dry = rng.standard_normal((n_sig, Ld)).astype(np.float32)
    dry[:, :Ld // 7] = 0.0                                              # leading silence, as the dataset's targets have
    t = np.arange(Lh)
    rir = (rng.standard_normal((n_sig, n_ch, Lh)) * np.exp(-6.9 * t / Lh)).astype(np.float32)
    rir[:, :, 5] += 1.0
    out_len = Ld if out_len is None else out_len
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    got = eng.rir_convolve(dry, rir, out_len).numpy()
    err = 0.0
    for i in range(n_sig):
        for c in range(n_ch):
            full = np.convolve(dry[i].astype(np.float64), rir[i, c].astype(np.float64))
            want = np.zeros(out_len)
            m = min(out_len, len(full))
            want[:m] = full[:m]
            err = max(err, float(np.max(np.abs(got[i, c] - want)) / np.max(np.abs(want))))
    assert err < tol, err
    return err


def check_iterated(make_engine, K=2, M=2, L=2304, iters=2, tol=1e-4):
    """disco_tango_enhance_iterated (DANSE-style extra step-2 iterations, BASELINE configs[4]) against the oracle's
    restatement of the same definition; iters = 1 must reproduce the plain two-step path."""
    from disco_amd import synth
    from oracle import tango_oracle as to
    y, s, n = synth.make_rooms_numpy(1, K=K, M=M, L=L)
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F).numpy()
    errs = {}
    for it in (1, iters):
        out, yf = eng.tango_enhance_iterated(y, m, iters=it)
        o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh', extra_iters=it - 1)
        errs[it] = max(relerr(yf.numpy()[0, k].T, o['yf'][k]) for k in range(K))
        assert errs[it] < tol, errs
    return errs


def check_ism_rir(make_engine, n_room=2, S=2, Q=3, max_order=5, rir_len=2048, seed=4, tol=5e-6):
    """disco_ism_rir against the float64 restatement of the same published algorithm (oracle/ism_oracle.py); pyroomacoustics
    itself is absent, so this is consistency of two independent statements of the formulas, not reference parity."""
    from oracle import ism_oracle as io
    rng = np.random.default_rng(seed)
    dims = np.stack([rng.uniform(3, 8, n_room), rng.uniform(3, 5, n_room), rng.uniform(2.5, 3, n_room)], 1).astype(np.float32)
    absorb = rng.uniform(0.2, 0.6, n_room).astype(np.float32)
    src = (rng.uniform(0.3, 0.7, (n_room, S, 3)) * dims[:, None]).astype(np.float32)
    mic = (rng.uniform(0.2, 0.8, (n_room, Q, 3)) * dims[:, None]).astype(np.float32)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    got = eng.ism_rir(dims, absorb, src, mic, max_order=max_order, rir_len=rir_len).numpy()
    assert np.all(np.isfinite(got))
    err = 0.0
    for r in range(n_room):
        for s in range(S):
            for q in range(Q):
                want = io.ism_rir(dims[r], float(absorb[r]), src[r, s], mic[r, q], max_order, 16000.0, 343.0, rir_len)
                err = max(err, float(np.max(np.abs(got[r, s, q] - want)) / np.max(np.abs(want))))
    assert err < tol, err
    # the direct path is the largest tap and sits at round(d / c * fs) + 40
    d = np.linalg.norm(src[0, 0] - mic[0, 0])
    assert abs(int(np.argmax(np.abs(got[0, 0, 0]))) - (int(round(d / 343.0 * 16000.0)) + 40)) <= 1
    return err


def check_solver_singular_noise(make_engine):
    """Numerically singular Rnn (coherent noise, silent channels): the solver must stay finite and bounded, and where the
    problem is still well posed (co-rank 1: one infinite generalized eigenvalue, clamped to 1e6 by the reference) it must
    agree with the reference's formulation (oracle intern_filter = scipy.linalg.eig path, internal_formulas.py:56-73)."""
    from oracle import mwf_oracle as mo
    rng = np.random.default_rng(0)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    errs = {}
    for P in (4, 7, 9, 15):
        for rank in (1, 2, P - 1):
            A = rng.standard_normal((P, rank)) + 1j * rng.standard_normal((P, rank))
            Rnn = (A @ A.conj().T).astype(np.complex64)
            B = rng.standard_normal((P, P + 2)) + 1j * rng.standard_normal((P, P + 2))
            Rss = (B @ B.conj().T / (P + 2)).astype(np.complex64)
            w, t1 = eng.gevd_mwf_r1(Rss[None], Rnn[None])
            w = w.numpy()[0]
            assert np.all(np.isfinite(w)) and np.abs(w).max() < 1e3, (P, rank, w)
            if rank == P - 1:
                wr, _ = mo.intern_filter(Rss, Rnn, mu=1, type='gevd', rank=1)
                errs[(P, rank)] = relerr(w, wr)
                assert errs[(P, rank)] < 1e-4, errs
    # an all-zero noise matrix and a silent channel
    for Rnn in (np.zeros((4, 4), np.complex64), np.diag([1, 0, 1, 1]).astype(np.complex64)):
        w, _ = eng.gevd_mwf_r1(np.eye(4, dtype=np.complex64)[None], Rnn[None])
        assert np.all(np.isfinite(w.numpy()))
    return errs


def check_node_sharded(make_engine, R=1, K=4, M=2, L=6000, world=2):
    """Node-sharded driver (z exchanged by an all-gather between the steps) == the single-GPU path, and == the oracle.
    The 'all-gather' here is a plain concatenation of the shards' z, run shard after shard in one process."""
    from disco_amd import synth
    from disco_amd.node_sharded import node_range, tango_enhance_node_sharded
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    full = make_engine(rooms=R, nodes=K, mics=M, length=L, staged_step2=True)
    T, F = full.T, full.F
    mask = full.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F).numpy()
    out_full, z_full, yf_full = full.tango_enhance(y, mask)
    out_full, z_full = out_full.numpy(), z_full.numpy()
    # pass 1: every shard's z (what the all-gather would deliver)
    shards = []
    for q in range(world):
        k0, kl = node_range(q, world, K)
        e = make_engine(rooms=R, nodes=K, mics=M, length=L)
        e.set_node_shard(k0, kl)
        shards.append((e, k0, kl))
    z_parts = {}

    def fake_gather_factory(q):
        def gather(z_local):
            z_parts[q] = z_local
            # the other shards' z: taken from the reference run (they would arrive over the wire)
            parts = [z_local if qq == q else z_full[:, qq * (K // world):(qq + 1) * (K // world)] for qq in range(world)]
            return np.concatenate(parts, axis=1)
        return gather
    worst = 0.0
    for q, (e, k0, kl) in enumerate(shards):
        out, yf, z_all = tango_enhance_node_sharded(e, y[:, k0:k0 + kl], mask[:, k0:k0 + kl], mask[:, k0:k0 + kl], fake_gather_factory(q))
        worst = max(worst, maxrel(out.numpy(), out_full[:, k0:k0 + kl]))
        # (the single-GPU run uses the fused STFT+covariance kernel, the shards the staged pair: same math, different
        #  accumulation order / fma contraction, so agreement is to fp32 rounding through the solver, not bit-for-bit)
        assert maxrel(z_parts[q], z_full[:, k0:k0 + kl]) < 5e-5
    assert worst < 1e-4, worst
    return worst


def check_apply_istft_sharded(make_engine, K=4, M=4, L=6000, n_fft=512, R=2, world=2, seed=8):
    """disco_apply_istft_fused on a NODE SHARD (k_apply_istft_wide with the shard's Kl nodes and the gathered z in rank-major blocks, the
    layout an all-gather delivers) against disco_apply + disco_istft on the same shard: the filtered spectra bit for bit, the samples to
    rounding (one inverse transform per frame pair instead of the staged kernel's own pairing); with and without the spectra going out;
    world = 1: the unsharded context (plain z layout).  Shapes: the narrow 4-mic ones a shard needs and a wide one."""
    from disco_amd.node_sharded import node_range
    rng = np.random.default_rng(seed)
    P = M + K - 1
    worst = 0.0
    for q in range(world):
        k0, kl = node_range(q, world, K)
        e = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        if world > 1:
            e.set_node_shard(k0, kl)
        T, F = e.T, e.F
        y = rng.standard_normal((R, kl, M, L)).astype(np.float32)
        X = e.stft(y.reshape(R * kl, M, L)).numpy().reshape(R, kl, T, F, M)
        w = (rng.standard_normal((R, kl, F, P)) + 1j * rng.standard_normal((R, kl, F, P))).astype(np.complex64)
        z_plain = (rng.standard_normal((R, K, T, F)) + 1j * rng.standard_normal((R, K, T, F))).astype(np.complex64)
        if world > 1:           # rank-major [W][R][Kl][T][F], consumed as it arrives
            z_arg = np.ascontiguousarray(z_plain.reshape(R, world, kl, T, F).transpose(1, 0, 2, 3, 4))
            e.set_z_blocks(kl)
        else:
            z_arg = z_plain
        yf_ref = e.apply(X, w, Z=z_arg)
        out_ref = e.istft(yf_ref.reshape(R * kl, T, F)).numpy().reshape(R, kl, L)
        yf_ref = yf_ref.numpy()
        yf_buf = e.empty((R, kl, T, F), np.complex64)
        out1 = e.apply_istft(X, w, z_arg, yf_out=yf_buf)
        assert out1 is not None, 'disco_apply_istft_fused is not built for this shape'
        out1 = out1.numpy().reshape(R, kl, L)
        assert np.array_equal(yf_buf.numpy(), yf_ref)
        out2 = e.apply_istft(X, w, z_arg).numpy().reshape(R, kl, L)
        assert np.array_equal(out1, out2)
        err = relerr(out1, out_ref)
        assert err < 3e-6, err
        worst = max(worst, err)
        if world > 1:
            e.set_z_blocks(K)
    return worst


def check_solver_vs_reference_golden(make_engine, golden_dir):
    """HIP solver against intern_filter outputs of the REFERENCE'S OWN CODE (tests/golden/intern_filter_ref.npz)."""
    import os
    g = np.load(os.path.join(golden_dir, 'intern_filter_ref.npz'))
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for i in range(int(g['n_cases'])):
        if str(g[f'c{i}_type']) != 'gevd':
            continue
        Rxx, Rnn = g[f'c{i}_Rxx'], g[f'c{i}_Rnn']
        w, t1 = eng.gevd_mwf_r1(Rxx[None].astype(np.complex64), Rnn[None].astype(np.complex64))
        # complex64 inputs: the reference itself solved in complex64 LAPACK -> 1e-4 class agreement;
        # complex128 inputs are rounded to complex64 at the ABI, same class.
        e = max(relerr(w.numpy()[0], g[f'c{i}_w']), relerr(t1.numpy()[0], g[f'c{i}_t1']))
        worst = max(worst, e)
        assert e < 2e-4, (i, e)
    return worst


def check_tango_end_to_end(make_engine, y, s, n, n_fft=512, mask='irm1', tol=1e-4, staged_step2=False, tuning=None):
    """Whole path through the C ABI vs the float64 oracle.  y, s, n: (R, K, M, L) float32.
    tuning = (stft_frames_per_wave, cov_chunks, step2_chunks, istft_pairs): pin the launch geometry (disco_set_tuning) to
    the one a large batch takes, and additionally check the `outputs=enhanced` call (no z / yf requested: the fused
    filter+iSTFT kernel, which is what bench.py times) against the same oracle.
    Returns the per-output worst relative errors."""
    R, K, M, L = y.shape
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft, mask=mask, staged_step2=staged_step2)
    if tuning is not None:
        eng.set_tuning(*tuning)
    T, F = eng.T, eng.F
    m_dev = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F)
    out, z, yf = eng.tango_enhance(y, m_dev)
    out_enh = eng.tango_enhance(y, m_dev, want_z=False, want_yf=False)[0].numpy()
    out, z, yf, m_gpu = out.numpy(), z.numpy(), yf.numpy(), m_dev.numpy()
    errs = {'mask': 0.0, 'mask_max': 0.0, 'z_y': 0.0, 'yf': 0.0, 'out': 0.0}
    for r in range(R):
        o = to.offline_tango_vec(y[r], s[r], n[r], vads=[mask, mask], n_fft=n_fft, hop=n_fft // 2,
                                 precision='f64', solver='eigh')
        for k in range(K):
            dm = np.abs(m_gpu[r, k].T - o['masks_z'][k])
            errs['mask'] = max(errs['mask'], float(np.percentile(dm, 99.9)))     # bulk: fp32 rounding class
            errs['mask_max'] = max(errs['mask_max'], float(dm.max()))            # tail: |N(f,t)| ~ 0 amplifies STFT rounding
            errs['z_y'] = max(errs['z_y'], relerr(z[r, k].T, o['z_y'][k]))
            errs['yf'] = max(errs['yf'], relerr(yf[r, k].T, o['yf'][k]))
            t_ref = so.istft(o['yf'][k], L, n_fft, n_fft // 2, work_dtype=np.float64)
            errs['out'] = max(errs['out'], relerr(out[r, k], t_ref))
            if out_enh is not None:
                errs['out_enhanced_only'] = max(errs.get('out_enhanced_only', 0.0), relerr(out_enh[r, k], t_ref))
    assert errs['mask'] < 2e-5 and errs['mask_max'] < 5e-3, errs
    assert errs['z_y'] < tol and errs['yf'] < tol and errs['out'] < tol and errs.get('out_enhanced_only', 0.0) < tol, errs
    return errs


def check_c5_full_length(make_engine, rooms=(0, 6, 64, 100, 141, 199), K=8, M=8, n_fft=1024, L=160000, iters=2, tol=1e-4):
    """BASELINE.json configs[4] at its real shape and length -- 8 nodes x 8 mics, 1024-point STFT, 10 s, two step-2 iterations -- on the
    first, middle and last room of bench.py's 200-room batch plus the four rooms that the 32-room sweep of round 5 found furthest from the
    oracle (profiles/r05_b_c5_32rooms_*.json: room 6 was at 1.49e-4 while the solvers rounded the combined sums to float32 at their door,
    3.5e-5 since they do not), against the float64 oracle at the north star's 1e-4.  The
    launch geometry is pinned to the one the 200-room batch takes (one frame chunk in the step-1 statistics; the room pass has none), so
    that every room goes through exactly the arithmetic it goes through in the bench.  The oracles run in worker processes while the
    GPU computes.  (The iterated scheme is an extension: the reference is strictly two-step, tango.py:1-7; the oracle defines it.)"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    from disco_amd import synth
    data = [synth.make_room_numpy(r, K=K, M=M, L=L)[:3] for r in rooms]
    y = np.stack([d[0] for d in data])
    s = np.stack([d[1] for d in data])
    n = np.stack([d[2] for d in data])
    R = len(rooms)
    # spawn, not fork: a forked worker would inherit this process's open GPU device files (its HIP runtime is up by now)
    with ProcessPoolExecutor(max_workers=R, mp_context=mp.get_context('spawn')) as pool:
        futs = [pool.submit(_c5_oracle_room, y[i], s[i, :, 0], n[i, :, 0], n_fft, iters) for i in range(R)]
        eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        eng.set_tuning(0, 1, 0, 0)
        m = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, eng.T, eng.F)
        out = eng.tango_enhance_iterated(y, m, iters=iters)[0].numpy()
        errs = {}
        for i, r in enumerate(rooms):
            ref = futs[i].result(timeout=1500)
            errs[r] = max(relerr(out[i, k], ref[k]) for k in range(K))
    assert max(errs.values()) < tol, errs
    return errs


def _c5_oracle_room(yr, s_ref, n_ref, n_fft, iters):
    s = np.zeros_like(yr)
    n = np.zeros_like(yr)
    s[:, 0] = s_ref                                       # the masks only look at the reference microphone (tango.py:338-342)
    n[:, 0] = n_ref
    o = to.offline_tango_vec(yr, s, n, vads=['irm1', 'irm1'], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh', extra_iters=iters - 1)
    return [so.istft(o['yf'][k], yr.shape[-1], n_fft, n_fft // 2, work_dtype=np.float64) for k in range(yr.shape[0])]


def check_iterated_outputs(make_engine, K, M, L, n_fft, iters, tol=1e-4):
    """disco_tango_enhance_iterated: STFT-domain AND time-domain outputs against the oracle's restatement of the same
    definition (offline_tango_vec(extra_iters=...)); iters = 1 must be the plain two-step path."""
    from disco_amd import synth
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    y, s, n = synth.make_rooms_numpy(1, K=K, M=M, L=L)
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L, n_fft=n_fft)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F)
    out, yf = eng.tango_enhance_iterated(y, m, iters=iters)
    o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh',
                             extra_iters=iters - 1)
    for k in range(K):
        assert relerr(yf.numpy()[0, k].T, o['yf'][k]) < tol
        ref = so.istft(o['yf'][k], L, n_fft, n_fft // 2, work_dtype=np.float64)
        assert relerr(out.numpy()[0, k], ref) < tol
    # iters = 1 must be the plain two-step path
    out1, _ = eng.tango_enhance_iterated(y, m, iters=1)
    out_ref, _, _ = eng.tango_enhance(y, m)
    assert relerr(out1.numpy(), out_ref.numpy()) < 1e-5
    return True


def check_reference_golden_scene(make_engine, golden_dir, scene):
    """HIP path against outputs of the REFERENCE'S OWN offline_tango (tests/golden/tango_ref_<scene>.npz)."""
    import os
    g = np.load(os.path.join(golden_dir, f'tango_ref_{scene}.npz'))
    K = int(g['K'])
    y = np.stack([g[f'y{k}'] for k in range(K)])[None]
    s = np.stack([g[f's{k}'] for k in range(K)])[None]
    n = np.stack([g[f'n{k}'] for k in range(K)])[None]
    R, K, M, L = y.shape
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F)
    out, z, yf = eng.tango_enhance(y, m)
    for k in range(K):
        assert np.abs(m.numpy()[0, k].T - g[f'masks_z{k}']).max() < 1e-3
        assert relerr(z.numpy()[0, k].T, g[f'z_y{k}']) < 1e-2
        assert relerr(yf.numpy()[0, k].T, g[f'yf{k}']) < 1e-2


def check_size_independent_properties(make_engine, R, K, M, L):
    """(i) iSTFT(STFT(x)) == x; (ii) the MWF output scales linearly with a common input gain (masks unchanged);
    (iii) batch independence: room r of a batch equals the same room processed alone, bit for bit."""
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    T, F = eng.T, eng.F
    m = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, T, F)
    out, z, yf = eng.tango_enhance(y, m)
    out2, z2, yf2 = eng.tango_enhance(2.0 * y, m)
    assert relerr(out2.numpy(), 2.0 * out.numpy()) < 1e-5            # (ii)
    eng1 = make_engine(rooms=1, nodes=K, mics=M, length=L)
    o1, _, _ = eng1.tango_enhance(y[R // 2:R // 2 + 1], m.numpy()[R // 2:R // 2 + 1])
    assert np.array_equal(o1.numpy()[0], out.numpy()[R // 2])                 # (iii) bit-identical
    X = eng.stft(y.reshape(R * K, M, L))
    xr = eng.istft(eng.stft(y[:, :, 0].reshape(R * K, 1, L)).reshape(R * K, T, F)).numpy()
    assert np.abs(xr - y[:, :, 0].reshape(R * K, L)).max() < 1e-5 * np.abs(y).max() + 1e-6   # (i)
    assert np.all(np.isfinite(out.numpy()))


def check_node_sharded_torch_one_rank(make_engine, device, backend, K=3, M=2, L=8192, iters=2):
    """tango_enhance_node_sharded_torch on a ONE-rank process group (the shard holds all K nodes; the all-gather is RCCL's /
    gloo's own single-rank path) against disco_tango_enhance_iterated on the same device: same staged kernels, so the
    outputs agree to rounding.  Exercises torch tensors as caller-owned z / yf buffers and disco_filter_head."""
    import socket
    import torch
    import torch.distributed as dist
    from disco_amd import synth
    from disco_amd.node_sharded import tango_enhance_node_sharded_torch
    R = 2
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    full = make_engine(rooms=R, nodes=K, mics=M, length=L)
    mask = full.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, full.T, full.F).numpy()
    own_group = not dist.is_initialized()
    if own_group:
        sk = socket.socket()
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group(backend, init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    try:
        errs = {}
        for it in (1, iters):
            out_ref, yf_ref = full.tango_enhance_iterated(y, mask, iters=it)
            eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
            eng.set_node_shard(0, K)
            yt = torch.from_numpy(y).to(device)
            mt = torch.from_numpy(mask).to(device)
            for overlap in (False, True):               # the plain call, and two half-batches with asynchronous all-gathers
                out, yf, z_all = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=it, overlap=overlap)
                assert yf.device.type == torch.device(device).type and tuple(z_all.shape) == (R, K, eng.T, eng.F)
                out_np = out.cpu().numpy() if hasattr(out, 'cpu') else out.numpy()
                errs[(it, overlap)] = (relerr(yf.cpu().numpy(), yf_ref.numpy()), relerr(out_np, out_ref.numpy()))
                assert max(errs[(it, overlap)]) < 1e-5, errs
    finally:
        if own_group:
            dist.destroy_process_group()
    return errs


def check_node_sharded_torch_want_yf(make_engine, device, backend, K=2, M=4, L=4096, iters=1):
    """tango_enhance_node_sharded_torch(want_yf=False) on a shape whose final filter + iSTFT run as one pass on the gathered z: the filtered
    spectra are not materialised (None comes back), the samples are those of the default call bit for bit; plain and with two half-batches."""
    import socket
    import torch
    import torch.distributed as dist
    from disco_amd import synth
    from disco_amd.node_sharded import tango_enhance_node_sharded_torch
    R = 3
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    mask = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, eng.T, eng.F).numpy()
    eng.set_node_shard(0, K)
    own_group = not dist.is_initialized()
    if own_group:
        sk = socket.socket()
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group(backend, init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    try:
        yt, mt = torch.from_numpy(y).to(device), torch.from_numpy(mask).to(device)
        for overlap in (False, True):
            out_a, yf_a, _ = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters, overlap=overlap)
            out_b, yf_b, _ = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters, overlap=overlap, want_yf=False)
            assert yf_a is not None and yf_b is None
            assert torch.equal(out_a.cpu(), out_b.cpu())
    finally:
        if own_group:
            dist.destroy_process_group()
    return True


def check_node_sharded_overlap_follows_parent(make_engine, device, backend, K=2, M=4, L=4096):
    """The half-batch engines of the overlapped node-sharded call carry the PARENT's configuration (round-5 ADVICE: they were built from the
    shape alone and solved with mu = 1 whatever the parent said): a parent with mu = 0.3, a non-default reference microphone, a pinned
    launch geometry and the LDS group solver gives the same samples with overlap=True as with overlap=False -- and other samples than a
    mu = 1 parent, so the comparison can tell."""
    import socket
    import torch
    import torch.distributed as dist
    from disco_amd import synth
    from disco_amd.node_sharded import tango_enhance_node_sharded_torch
    R = 3
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    own_group = not dist.is_initialized()
    if own_group:
        sk = socket.socket()
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group(backend, init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1)
    try:
        outs = {}
        for mu in (0.3, 1.0):
            eng = make_engine(rooms=R, nodes=K, mics=M, length=L, mu=mu, ref_mic=1)
            mask = eng.mask_oracle(s[:, :, 1].reshape(R * K, L), n[:, :, 1].reshape(R * K, L)).reshape(R, K, eng.T, eng.F).numpy()
            eng.set_node_shard(0, K)
            eng.set_tuning(8, 2, 2, 4)
            eng.set_option('solve_thread', 0)
            yt, mt = torch.from_numpy(y).to(device), torch.from_numpy(mask).to(device)
            for overlap in (False, True):
                out, _, _ = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=2, overlap=overlap)
                outs[(mu, overlap)] = (out.cpu().numpy() if hasattr(out, 'cpu') else out.numpy()).copy()
            kids = eng._ns_halves[1]
            assert all(abs(k.cfg.mu - mu) < 1e-7 and k.cfg.ref_mic == 1 and k._tuning == (8, 2, 2, 4) and k.get_option('solve_thread') == 0
                       and k.stream == eng.stream for k in kids)
            # an option changed on the parent AFTER the children exist reaches them on the next call
            eng.set_option('solve_thread', 1)
            tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=1, overlap=True)
            assert all(k.get_option('solve_thread') == 1 for k in eng._ns_halves[1])
        e_same = relerr(outs[(0.3, True)], outs[(0.3, False)])
        e_mu = relerr(outs[(0.3, False)], outs[(1.0, False)])
        assert e_same < 1e-5 and e_mu > 1e-2, (e_same, e_mu)
    finally:
        if own_group:
            dist.destroy_process_group()
    return e_same, e_mu


def check_solver_sizes(make_engine, sizes=range(1, 17), n=300, tol=2e-6):
    """P = 1..16 (C5 needs 15): HIP float64 solver vs the numpy eigh closed form on rank-1-plus-noise pencils."""
    rng = np.random.default_rng(11)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for P in sizes:
        T = 6 * P + 5
        a = rng.standard_normal((n, P, 1)) + 1j * rng.standard_normal((n, P, 1))
        X = a * (rng.standard_normal((n, 1, T)) + 1j * rng.standard_normal((n, 1, T))) + 0.3 * (
            rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T)))
        Nn = rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T))
        Rxx = (X @ X.conj().transpose(0, 2, 1) / T).astype(np.complex64)
        Rnn = (Nn @ Nn.conj().transpose(0, 2, 1) / T).astype(np.complex64)
        w, t1 = eng.gevd_mwf_r1(Rxx, Rnn)
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
        e = max(relerr(w.numpy(), wr), relerr(t1.numpy(), t1r))
        assert e < tol, (P, e)
        worst = max(worst, e)
    return worst


def _pencil_with_spectrum(rng, n, P, d):
    """n Hermitian pencils (Rxx, Rnn) whose generalized eigenvalues are exactly d (descending), built in float64."""
    A = rng.standard_normal((n, P, P)) + 1j * rng.standard_normal((n, P, P))
    Rnn = A @ A.conj().transpose(0, 2, 1) / P + 0.5 * np.eye(P)
    L = np.linalg.cholesky(Rnn)
    V, _ = np.linalg.qr(rng.standard_normal((n, P, P)) + 1j * rng.standard_normal((n, P, P)))
    C = (V * np.asarray(d)[None, None, :]) @ V.conj().transpose(0, 2, 1)
    Rxx = L @ C @ L.conj().transpose(0, 2, 1)
    return Rxx, Rnn


def check_solver_small_gap(make_engine, sizes=(2, 4, 7, 15)):
    """Pencils whose two largest generalized eigenvalues are close (d1/d0 up to 0.9999): the dominant-pair iteration must
    keep going until it has separated them.  The bound scales with the conditioning of the eigenvector, 1 / (1 - d1/d0):
    the float32 rounding of the INPUTS alone moves v0 by ~1e-7 / gap, so both solvers are compared on the same complex64
    inputs.  Also: an exactly repeated top eigenvalue and non-finite input must give finite / contained results."""
    rng = np.random.default_rng(5)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    out = {}
    for P in sizes:
        for ratio in (0.9, 0.99, 0.999, 0.9999):
            d = np.concatenate([[1.0, ratio], ratio * rng.uniform(0.0, 0.9, max(P - 2, 0))])[:P]
            d = 3.0 * np.sort(d)[::-1]
            Rxx, Rnn = _pencil_with_spectrum(rng, 64, P, d)
            w64, _, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
            Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
            w, t1 = eng.gevd_mwf_r1(Rxx, Rnn)
            wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
            e = max(relerr(w.numpy(), wr), relerr(t1.numpy(), t1r))
            inherent = relerr(wr, w64)                  # what rounding the pencil to complex64 -- the solver's input format -- costs
            out[(P, ratio)] = (e, inherent)
            assert e < 2e-6, (P, ratio, e, inherent)    # same inputs on both sides: float64 accuracy regardless of the gap
    # one slow pencil (d1/d0 = 0.99999, ~20 squarings) in a batch of quick ones whose Rxx is NOT exactly Hermitian (the two
    # triangles differ at float32 rounding level, as in the online kernel where every lane accumulates its own row): the
    # quick ones wait in the same wave and must come out untouched.  (A normaliser that ignores the imaginary part of
    # tr(B^2) lets the phase of the common complex scale double per squaring: this case then fails on the whole wave.)
    for P in (4, 7):
        n = 64
        d_fast = np.concatenate([[1.0, 0.6], 0.6 * rng.uniform(0.0, 0.9, P - 2)])
        Rxx, Rnn = _pencil_with_spectrum(rng, n, P, 2.0 * np.sort(d_fast)[::-1])
        d_slow = np.concatenate([[1.0, 0.99999], 0.5 * rng.uniform(0.0, 0.9, P - 2)])
        Rs, Rn = _pencil_with_spectrum(rng, 1, P, 2.0 * np.sort(d_slow)[::-1])
        Rxx[9], Rnn[9] = Rs[0], Rn[0]
        skew = rng.standard_normal((n, P, P)) + 1j * rng.standard_normal((n, P, P))
        skew = (skew - skew.conj().transpose(0, 2, 1)) * 2e-7 * np.abs(Rxx).mean()
        Rxx32, Rnn32 = (Rxx + skew).astype(np.complex64), Rnn.astype(np.complex64)
        w, t1 = eng.gevd_mwf_r1(Rxx32, Rnn32)
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(0.5 * (Rxx32 + Rxx32.conj().transpose(0, 2, 1)), Rnn32, 1.0)
        quick = np.arange(n) != 9
        e = max(relerr(w.numpy()[quick], wr[quick]), relerr(t1.numpy()[quick], t1r[quick]))
        out[(P, 'mixed')] = e
        assert e < 5e-6, (P, e)                         # 2e-7 of skew / a relative gap of 0.4
        assert np.all(np.isfinite(w.numpy().view(np.float32)))
    # exactly repeated top eigenvalue: any vector of the dominant plane is a valid v0; the gain d0/(d0+mu) is unique
    P = 4
    Rxx, Rnn = _pencil_with_spectrum(rng, 8, P, [2.0, 2.0, 0.5, 0.1])
    w, t1 = eng.gevd_mwf_r1(Rxx.astype(np.complex64), Rnn.astype(np.complex64))
    w, t1 = w.numpy(), t1.numpy()
    assert np.all(np.isfinite(w.view(np.float32))) and np.all(np.isfinite(t1.view(np.float32)))
    ratio = np.linalg.norm(w, axis=-1) / np.linalg.norm(t1, axis=-1)
    assert np.abs(ratio - 2.0 / 3.0).max() < 1e-5, ratio
    # a NaN pencil next to good ones must not contaminate its neighbours (groups share waves and LDS)
    Rxx, Rnn = _pencil_with_spectrum(rng, 16, P, [2.0, 1.0, 0.5, 0.1])
    Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
    wr, _, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
    Rxx[5] = np.nan
    w, _ = eng.gevd_mwf_r1(Rxx, Rnn)
    w = w.numpy()
    good = np.arange(16) != 5
    assert relerr(w[good], wr[good]) < 2e-6
    return out


def _indefinite_spectra(rng, P):
    """Generalized spectra (descending) of the indefinite-pencil check, by case.  (a)-(c) are what the squaring alone gets wrong: the
    dominant eigenvalue (largest |d|) is negative, the first tau = tr(B^2) test is fooled, or the trace is not positive."""
    cases = {'d_psd': np.concatenate([[2.0], rng.uniform(0.0, 1.2, P - 1)])}
    if P == 1:
        cases['e_nonpositive'] = np.array([-0.7])
        return {k: np.sort(v)[::-1] for k, v in cases.items()}
    cases['a_dominant_negative'] = np.concatenate([[0.5], rng.uniform(-1.5, 0.3, P - 2), [-2.0]])
    for r in (0.3, 0.6, 0.9):                           # top positive and dominant, the next largest |d| negative: |d1 / d0| = r
        cases[f'b_negative_second_{r}'] = np.concatenate([[3.0], 3.0 * r * rng.uniform(-0.9, 0.9, P - 2), [-3.0 * r]])
    m = P - 2
    if m >= 3:
        # {1, s (m times), -0.9} with tau_0 = (1.81 + m s^2) / (0.1 + m s)^2 = 0.9: the first test stops the squaring at once, with the
        # top pair unresolved and tau_0 <= 1
        a, b, c = 0.9 * m * m - m, 0.18 * m, 0.009 - 1.81
        sv = (-b + np.sqrt(b * b - 4 * a * c)) / (2 * a)
        cases['b_first_test_fooled'] = np.concatenate([[1.0], np.full(m, sv), [-0.9]])
    cases['c_negative_trace'] = np.concatenate([[0.5], rng.uniform(-2.0, -0.6, P - 1)])
    cases['e_nonpositive'] = rng.uniform(-2.0, -0.1, P)
    return {k: np.sort(v)[::-1] for k, v in cases.items()}


def check_solver_indefinite(make_engine, sizes=range(1, 17), option=None, value=None, per_case=9, cross=2, seed=29):
    """Indefinite Hermitian pencils (Rxx = Ryy - Rnn, as a drop-in caller of intern_filter passes them): the solver must return the TOP
    (algebraically largest) generalized eigenpair, clamped, as internal_formulas.py:56-73 does -- not the dominant one, which is what
    repeated squaring finds.  Every case of _indefinite_spectra for each P, mixed in one launch whose size is not a multiple of the
    pencils per block or wave; `option` = `value` picks the route (solve_thread 0/1 for P = 5..8, solve_dpp 0/1 for P = 9..16).
    Reference: the float64 closed form on the same complex64 inputs, itself checked against mo.intern_filter on `cross` pencils per case.
    Bar: 2e-6 / (1 - gap), gap = 1 - (d0 - d1) / max|d| -- d1 / d0 for a PSD spectrum, as in check_solver_small_gap.  All d <= 0 (case e):
    every eigenvalue clamps to eps, so only |w| <= 1e-10 |t1| and finiteness are asserted, not the direction."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    if option is not None:
        eng.set_option(option, value)
        assert eng.get_option(option) == value
    out = {}
    for P in sizes:
        spectra = _indefinite_spectra(rng, P)
        names, Rxx, Rnn = [], [], []
        for name, d in spectra.items():
            A, B = _pencil_with_spectrum(rng, per_case, P, d)
            names += [name] * per_case
            Rxx.append(A)
            Rnn.append(B)
        Rxx, Rnn, names = np.concatenate(Rxx), np.concatenate(Rnn), np.array(names)
        if len(names) % 4 == 0:                         # ragged last block / wave for every route
            Rxx, Rnn, names = Rxx[:-1], Rnn[:-1], names[:-1]
        order = rng.permutation(len(names))
        Rxx, Rnn, names = Rxx[order].astype(np.complex64), Rnn[order].astype(np.complex64), names[order]
        w, t1 = eng.gevd_mwf_r1(Rxx, Rnn, mu=1.0)
        w, t1 = w.numpy().astype(np.complex128), t1.numpy().astype(np.complex128)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(t1)), P
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
        for name, d in spectra.items():
            sel = names == name
            if name.startswith('e_'):
                ratio = np.linalg.norm(w[sel], axis=-1) / np.linalg.norm(t1[sel], axis=-1)
                assert ratio.max() <= 1e-10, (P, name, ratio.max())
                out[(P, name)] = float(ratio.max())
                continue
            for i in np.flatnonzero(sel)[:cross]:       # the closed form is the reference's own branch on a Hermitian pencil
                wi, (t1i, _) = mo.intern_filter(Rxx[i].astype(np.complex128), Rnn[i].astype(np.complex128), mu=1, type='gevd', rank=1)
                assert relerr(wi, wr[i]) < 1e-9 and relerr(t1i, t1r[i]) < 1e-9, (P, name, relerr(wi, wr[i]))
            gap = 1.0 - (d[0] - d[1]) / np.abs(d).max() if P > 1 else 0.0
            bar = 2e-6 / (1.0 - gap)
            e = max((np.linalg.norm(w[sel] - wr[sel], axis=-1) / np.linalg.norm(wr[sel], axis=-1)).max(),
                    (np.linalg.norm(t1[sel] - t1r[sel], axis=-1) / np.linalg.norm(t1r[sel], axis=-1)).max())
            out[(P, name)] = float(e)
            assert e < bar, (P, option, value, name, e, bar)
    return out


def _mwf_variant_ref(Rxx, Rnn, mu, type):
    """mo.intern_filter's 'mwf' / 'r1-mwf' branches restated for (..., P, P) Hermitian float64 batches: np.linalg.lstsq of a regular
    matrix is its solve; 'r1-mwf' keeps the eigenpair of D.max() over the real eigenvalues (the algebraically largest) and scales it by |Dmax|."""
    Rxx, Rnn = Rxx.astype(np.complex128), Rnn.astype(np.complex128)
    if type == 'mwf':
        return np.linalg.solve(Rnn + Rxx, Rxx[..., :, :1])[..., 0]
    D, X = np.linalg.eigh(Rxx)
    x = X[..., :, -1]
    R1 = np.abs(D[..., -1])[..., None, None] * x[..., :, None] * np.conjugate(x)[..., None, :]
    Pm = np.linalg.solve(Rnn, R1)
    return Pm[..., :, 0] / (mu + np.trace(Pm, axis1=-2, axis2=-1))[..., None]


def check_mwf_variants(make_engine, sizes=range(1, 17), n=37, seed=31, tol=2e-6):
    """disco_mwf_filter ('mwf' and 'r1-mwf', csrc/k_mwf_variants) on (2, n) batches -- every slot of a block carries a pencil, the last
    block is ragged -- at mu 1 and 0.3, with PSD, indefinite (top positive, dominant negative) and negative-definite Rxx mixed in one
    launch.  Rnn + Rxx stays positive definite (Rnn covers Rxx's negative part), as the 'mwf' branch's Cholesky needs.  Reference:
    _mwf_variant_ref in float64 on the same complex64 inputs, checked against mo.intern_filter itself on a few pencils; bar: `tol`
    relative per pencil."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    out = {}
    for P in sizes:
        N = 2 * n
        kind = rng.integers(0, 3, N)                    # 0: PSD, 1: indefinite, 2: negative definite
        d = np.empty((N, P))
        for i in range(N):
            if kind[i] == 0:
                d[i] = np.concatenate([[2.0], rng.uniform(0.0, 1.2, P - 1)])
            elif kind[i] == 1:
                d[i] = np.concatenate([[0.5], rng.uniform(-1.5, 0.3, P - 2), [-2.0]]) if P > 1 else [-0.7]
            else:
                d[i] = np.concatenate([[-0.3], rng.uniform(-2.0, -0.8, P - 1)])
        U, _ = np.linalg.qr(rng.standard_normal((N, P, P)) + 1j * rng.standard_normal((N, P, P)))
        Uh = U.conj().transpose(0, 2, 1)
        Rxx = (U * d[:, None, :]) @ Uh
        A = rng.standard_normal((N, P, P)) + 1j * rng.standard_normal((N, P, P))
        Rnn = A @ A.conj().transpose(0, 2, 1) / P + 0.5 * np.eye(P) + (U * np.maximum(-d, 0.0)[:, None, :]) @ Uh
        Rxx = Rxx.reshape(2, n, P, P).astype(np.complex64)
        Rnn = Rnn.reshape(2, n, P, P).astype(np.complex64)
        for typ in ('mwf', 'r1-mwf'):
            for mu in (1.0, 0.3):
                w = eng.mwf_filter(Rxx, Rnn, type=typ, mu=mu).numpy().astype(np.complex128)
                assert w.shape == (2, n, P)
                wr = _mwf_variant_ref(Rxx, Rnn, mu, typ)
                for b, i in ((0, 0), (1, n - 1)):
                    wi, _ = mo.intern_filter(Rxx[b, i].astype(np.complex128), Rnn[b, i].astype(np.complex128), mu=mu, type=typ)
                    assert relerr(wi, wr[b, i]) < 1e-9, (P, typ, mu, relerr(wi, wr[b, i]))
                e = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
                out[(P, typ, mu)] = float(e.max())
                assert np.all(np.isfinite(w)) and e.max() < tol, (P, typ, mu, kind.reshape(2, n)[np.unravel_index(e.argmax(), e.shape)], e.max())
    return out


def check_solver_routes(make_engine, sizes=(9, 12, 15, 16), n=37, option='solve_dpp'):
    """9 <= P <= 16: the register / DPP solver (option "solve_dpp", csrc/k_solve_dpp.h) -- or, option = 'solve_thread', 5 <= P <= 8: one
    thread per pencil (csrc/k_solve_small.h) -- against the LDS group solver on the same pencils: covariance-like, nearly singular noise (a
    broken pivot), a small gap, Rxx = 0, and a batch size that leaves lanes of the last wave without a pencil; both against the float64
    closed form where that is well conditioned."""
    rng = np.random.default_rng(23)
    a = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    b = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    a.set_option(option, 1)
    b.set_option(option, 0)
    assert a.get_option(option) == 1 and b.get_option(option) == 0
    out = {}
    for P in sizes:
        T = 4 * P
        X = (rng.standard_normal((n, P, 1)) + 1j * rng.standard_normal((n, P, 1))) * (rng.standard_normal((n, 1, T)) + 1j * rng.standard_normal((n, 1, T))) \
            + 0.3 * (rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T)))
        Nn = rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T))
        Rxx = (X @ X.conj().transpose(0, 2, 1) / T)
        Rnn = (Nn @ Nn.conj().transpose(0, 2, 1) / T)
        Rnn[1] = Rnn[1][:, :1] @ Rnn[1][:, :1].conj().T + 1e-9 * np.eye(P)          # rank 1: every pivot after the first breaks down
        Rxx[2] = 0.0                                                               # nothing to enhance
        Rg, Ng = _pencil_with_spectrum(rng, 1, P, [1.0, 0.999] + [0.3] * (P - 2))   # a gap of 1e-3
        Rxx[3], Rnn[3] = Rg[0], Ng[0]
        Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
        wa, ta = a.gevd_mwf_r1(Rxx, Rnn)
        wb, tb = b.gevd_mwf_r1(Rxx, Rnn)
        wa, ta, wb, tb = wa.numpy(), ta.numpy(), wb.numpy(), tb.numpy()
        assert np.all(np.isfinite(wa.view(np.float32))) and np.all(np.isfinite(ta.view(np.float32))), P
        reg = np.ones(n, bool)
        reg[[1, 3]] = False                                                        # compared with their own bars below
        e_ab = max(relerr(wa[reg], wb[reg]), relerr(ta[reg], tb[reg]))
        reg[2] = False                                                             # (w = 0: no relative error)
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx[reg], Rnn[reg], 1.0)
        e_ref = max(relerr(wa[reg], wr), relerr(ta[reg], t1r))
        assert e_ab < 1e-6 and e_ref < 2e-6, (P, e_ab, e_ref)
        assert np.abs(wa[2]).max() < 1e-12
        e_gap = relerr(wa[3], wb[3])
        assert e_gap < 2e-3, (P, e_gap)                                            # float32 inputs move v0 by ~1e-7 / gap in either solver
        assert np.abs(wa[1]).max() < 1e3 and relerr(wa[1], wb[1]) < 1e-3, (P, wa[1], wb[1])
        out[P] = (e_ab, e_ref, e_gap)
    return out


def check_solver_degenerate(make_engine):
    """Rss = 0 (mask 0 everywhere): eigenvalue clamps to eps -> w ~ 0, finite (internal_formulas.py:59-62)."""
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    for P in (1, 4, 7, 15):
        Rnn = np.eye(P, dtype=np.complex64)[None].repeat(3, 0)
        Rss = np.zeros((3, P, P), np.complex64)
        w, t1 = eng.gevd_mwf_r1(Rss, Rnn)
        assert np.all(np.isfinite(w.numpy().view(np.float32))) and np.abs(w.numpy()).max() < 1e-12


def check_pk_selftest(make_engine, n=4096, seed=11):
    """csrc/pk.h: every packed complex operation through the v_pk_* instruction forms (on the emulated build: their C++
    statement) must equal its C++ statement bit for bit, and both must mean what the operation's name says (NumPy)."""
    rng = np.random.default_rng(seed)
    a, b, c = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for _ in range(3)]
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    hw, ref = eng.selftest_pk(a, b, c)
    hw, ref = hw.numpy(), ref.numpy()
    assert np.array_equal(hw.view(np.uint32), ref.view(np.uint32)), 'instruction forms differ from their C++ statement'
    A, B, C_ = a.astype(np.complex128), b.astype(np.complex128), c.astype(np.complex128)
    h = 0.70710678118654752440
    kt = 0.92387953251128675613 - 0.38268343236508977173j
    want = [A + np.conj(B), -1j * (A - np.conj(B)), A - 1j * B, A + 1j * B, np.conj(A + 1j * B), (1 - 1j) * A, (1 + 1j) * A,
            A * B, A * kt, A * np.conj(B), C_ + np.conj(A) * B, C_ + h * A, C_ - h * A, A * B.real, A * B.imag, C_ + A * B.imag, C_ + A * B,
            A.real * B.real + 1j * A.imag * B.imag, C_ + A.real * B.real + 1j * A.imag * B.imag, C_ + A.real * B, C_ + 1j * A.imag * B,
            C_ - 1j * A.imag * B, C_ + A * B.real]
    errs = {}
    for q, w in enumerate(want):
        errs[q] = float(np.abs(hw[:, q] - w).max() / np.abs(w).max())
    assert max(errs.values()) < 1e-6, errs
    return errs


def check_room_selftest(make_engine, n=4096, seed=17):
    """csrc/k_room.h: lds_dma16 / lds_dma4 + vm_wait_all, lane_swap_add<32 / 16> and lane_swap_add64<32 / 16> through their instruction forms (on the emulated build:
    their C++ twins) must equal plain loads / the __shfl_xor statement bit for bit, and mean what they say (NumPy)."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n).astype(np.float32)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    hw, ref = eng.selftest_room(src)
    hw, ref = hw.numpy(), ref.numpy()
    assert np.array_equal(hw.view(np.uint32), ref.view(np.uint32)), 'instruction forms differ from their plain statement'
    blk = src.reshape(-1, 256)
    lane = np.arange(64)
    perm = (lane * 5 + 3) & 63
    g = blk.reshape(-1, 64, 4)[:, perm]                                    # the granule lane l fetched
    a, b = blk[:, :64], blk[:, 64:128]
    want = np.stack([g[..., 0] + np.float32(2) * g[..., 1] + np.float32(3) * g[..., 2] + np.float32(5) * g[..., 3], blk[:, perm],
                     np.where(lane & 32, b[:, lane ^ 32] + b, a + a[:, lane ^ 32]), np.where(lane & 16, b[:, lane ^ 16] + b, a + a[:, lane ^ 16])], axis=-1)
    err = float(np.abs(hw.reshape(-1, 64, 6)[..., :4] - want).max())
    assert err < 1e-5, err
    # rows 4, 5: the float64 swaps (lane_swap_add64), operands da = a (1 + 2^-23) + 1e-9 b, db = b (1 - 2^-23) - 1e-9 a; head + 1e6 x remainder
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    da, db = a64 * 1.0000001192092896 + b64 * 1e-9, b64 * 0.9999998807907104 - a64 * 1e-9
    for row, bit in ((4, 32), (5, 16)):
        d = np.where(lane & bit, db[:, lane ^ bit] + db, da + da[:, lane ^ bit])
        h = d.astype(np.float32)
        w64 = ((d - h.astype(np.float64)).astype(np.float32) * np.float32(1e6) + h)
        e64 = float(np.abs(hw.reshape(-1, 64, 6)[..., row] - w64).max())
        assert e64 < 1e-5, (row, e64)
    return err


def check_dpp_selftest(make_engine, n=1024, seed=13):
    """csrc/dpp64.h: the float64 DPP row-broadcast forms must equal __shfl + the plain fused multiply-adds bit for bit, and both must
    mean what the helper says (NumPy): lane i of a 16-lane row reads entries of the other lanes of ITS row."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    hw, ref = eng.selftest_dpp(a, b)
    hw, ref = hw.numpy(), ref.numpy()
    assert np.array_equal(hw.view(np.uint64), ref.view(np.uint64)), 'instruction forms differ from __shfl + plain statements'
    A, B = a.reshape(-1, 16), b.reshape(-1, 16)
    bc = lambda v, k: np.repeat(v[:, k:k + 1], 16, axis=1)
    want = [A + bc(B, 0) * A, A - bc(B, 5) * A, A - A * np.conj(bc(B, 9)), A + np.conj(A) * bc(B, 15), A - np.conj(A) * bc(B, 3),
            bc(B.real, 7) + 1j * bc(B.imag, 12), np.repeat(A.real.sum(1, keepdims=True), 16, 1) + 1j * np.repeat(B.imag.sum(1, keepdims=True), 16, 1),
            bc(A.real, 6) + bc(B, 6) * A]
    errs = {}
    for q, w in enumerate(want):
        errs[q] = float(np.abs(hw[:, q] - w.reshape(-1)).max() / np.abs(w).max())
    assert max(errs.values()) < 1e-14, errs
    return errs


def check_no_allocation_in_compute_calls(make_engine, K=3, M=2, L=6000, n_fft=512):
    """include/disco_hip.h: disco_create sizes the partial-sum blocks, disco_reserve(ctx, 1|2) the context's own workspace;
    afterwards no whole-path or stage call allocates (disco_owned_bytes is unchanged across every one of them), also after
    disco_set_tuning picks another geometry.  With DISCO_FLAG_LAZY_SCRATCH nothing is owned until the first covariance call."""
    from disco_amd import synth, _lib
    y, s, n = synth.make_rooms_numpy(2, K=K, M=M, L=L)
    eng = make_engine(rooms=2, nodes=K, mics=M, length=L, n_fft=n_fft)
    assert eng.owned_bytes() > 0
    eng.reserve(2)
    own = eng.owned_bytes()
    assert own >= eng.workspace_bytes()
    m = eng.mask_oracle(s[:, :, 0].reshape(2 * K, L), n[:, :, 0].reshape(2 * K, L)).reshape(2, K, eng.T, eng.F)
    eng.tango_enhance(y, m)
    eng.tango_enhance(y, m, want_z=False, want_yf=False)
    eng.tango_enhance_iterated(y, m, iters=2)
    eng.tango_reference(y, s, n)
    X = eng.stft(y.reshape(2 * K, M, L))
    eng.cov_masked(X.reshape(2, K, eng.T, eng.F, M), m)
    assert eng.owned_bytes() == own, (eng.owned_bytes(), own)
    for tuning in ((8, 8, 8, 2), (80, 1, 1, 64), (0, 0, 0, 0)):
        eng.set_tuning(*tuning)
        own_t = eng.owned_bytes()
        assert own_t >= own
        eng.tango_enhance(y, m)
        eng.tango_enhance_iterated(y, m, iters=2)
        assert eng.owned_bytes() == own_t, (tuning, eng.owned_bytes(), own_t)
    # opt-out: nothing is owned until a covariance call needs it
    lazy = make_engine(rooms=2, nodes=K, mics=M, length=L, n_fft=n_fft, lazy_scratch=True)
    assert lazy.owned_bytes() == 0
    lazy.stft(y.reshape(2 * K, M, L))
    assert lazy.owned_bytes() == 0
    out_lazy = lazy.tango_enhance(y, m.numpy())[0].numpy()
    assert lazy.owned_bytes() > 0
    eng.set_tuning(0, 0, 0, 0)
    assert np.array_equal(out_lazy, eng.tango_enhance(y, m)[0].numpy())
    return own


def check_room_cov(make_engine, K=2, M=8, L=6000, n_fft=512, iters=2, R=2, tuning=None, tol=1e-4):
    """k_room_cov (csrc/k_room.h: z of every node + the step-2 statistics of every node of a room from ONE pass over X, wide
    shapes P = M + K - 1 > 8) against (a) the route it replaces -- disco_apply + the split covariance kernels, selected with
    disco_set_option("room_cov", 0) -- and (b) the float64 oracle; both whole-path entry points.  The routes run on SEVERAL
    contexts alive at the same time (options are per context, not process-global), and the stage names say which route ran."""
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    if tuning is not None:
        eng.set_tuning(*tuning)
    m = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, eng.T, eng.F)
    res = {}
    # '1': the default (the persistent pass on the LDS-DMA ring), '0': the staged route
    engines = {}
    for mode, cov in (('1', 1), ('0', 0)):
        e = eng if mode == '1' else make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        if mode != '1' and tuning is not None:
            e.set_tuning(*tuning)
        e.set_option('room_cov', cov)
        engines[mode] = e
    m_np = m.numpy()
    want_stage = {'1': 'room_cov2', '0': 'cov2'}
    for mode, e in engines.items():
        mm = m if e is eng else m_np
        e.stage_timing(True)
        out_i, yf_i = e.tango_enhance_iterated(y, mm, iters=iters)
        stages = set(e.stage_report())
        e.stage_timing(False)
        assert want_stage[mode] in stages and not (set(want_stage.values()) - {want_stage[mode]}) & stages, (mode, stages)
        out_e, z_e, yf_e = e.tango_enhance(y, mm)
        res[mode] = (out_i.numpy(), yf_i.numpy(), out_e.numpy(), z_e.numpy(), yf_e.numpy())
    errs = {}
    for q, name in enumerate(('out_iter', 'yf_iter', 'out', 'z_y', 'yf')):
        for mode in res:
            if mode != '0':
                errs[f'{name}_{mode}_vs_staged'] = max(relerr(res[mode][q][r, k], res['0'][q][r, k]) for r in range(R) for k in range(K))
    assert max(errs.values()) < 2e-5, errs
    for r in range(R):
        for it_, (o_idx, yf_idx) in ((iters, (0, 1)), (1, (2, 4))):
            o = to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh',
                                     extra_iters=it_ - 1)
            for k in range(K):
                errs['yf_oracle'] = max(errs.get('yf_oracle', 0.0), relerr(res['1'][yf_idx][r, k].T, o['yf'][k]))
                ref = so.istft(o['yf'][k], L, n_fft, n_fft // 2, work_dtype=np.float64)
                errs['out_oracle'] = max(errs.get('out_oracle', 0.0), relerr(res['1'][o_idx][r, k], ref))
                if it_ == 1:
                    errs['z_oracle'] = max(errs.get('z_oracle', 0.0), relerr(res['1'][3][r, k].T, o['z_y'][k]))
    assert errs['yf_oracle'] < tol and errs['out_oracle'] < tol and errs['z_oracle'] < tol, errs
    return errs


def check_apply_istft_wide(make_engine, K=2, M=8, L=6000, n_fft=1024, iters=2, R=2, pairs=0, tol=1e-4, oracle=True):
    """k_apply_istft_wide (csrc/k_fused.h: the final filter + iSTFT of the wide shapes in one pass, stage "apply2_istft") against the route
    it replaces (disco_set_option("fuse_wide_istft", 0): "apply2" + "istft") and the float64 oracle, with and without the filtered spectra
    requested, both whole-path entry points.  yf must be BIT-identical between the routes (same arithmetic per bin); the samples differ by
    the rounding of which two frames share an inverse transform."""
    from disco_amd import synth
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    res = {}
    for mode in ('fused', 'staged'):
        e = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
        e.set_option('fuse_wide_istft', 1 if mode == 'fused' else 0)
        if pairs:
            e.set_tuning(0, 0, 0, pairs)
        m = e.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, e.T, e.F)
        e.stage_timing(True)
        out_i, yf_i = e.tango_enhance_iterated(y, m, iters=iters)
        stages = set(e.stage_report())
        e.stage_timing(False)
        assert ('apply2_istft' in stages) == (mode == 'fused') and ('istft' in stages) == (mode == 'staged'), (mode, stages)
        out_e, _, yf_e = e.tango_enhance(y, m)
        out_n, _, none_ = e.tango_enhance(y, m, want_z=False, want_yf=False)
        assert none_ is None
        res[mode] = (out_i.numpy(), yf_i.numpy(), out_e.numpy(), yf_e.numpy(), out_n.numpy())
    f, g = res['fused'], res['staged']
    assert np.array_equal(f[1], g[1]) and np.array_equal(f[3], g[3]), 'yf differs between the one-pass and the staged route'
    assert np.array_equal(f[2], f[4]), 'the samples depend on whether yf was requested'
    errs = {'out_iter_vs_staged': max(relerr(f[0][r, k], g[0][r, k]) for r in range(R) for k in range(K)),
            'out_vs_staged': max(relerr(f[2][r, k], g[2][r, k]) for r in range(R) for k in range(K))}
    assert max(errs.values()) < 2e-6, errs
    if not oracle:              # (clips of fewer frames than channels: singular statistics, the oracle's Cholesky refuses them)
        return errs
    for r in range(R):
        for it_, (o_idx, yf_idx) in ((iters, (0, 1)), (1, (2, 3))):
            o = to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], n_fft=n_fft, hop=n_fft // 2, precision='f64', solver='eigh',
                                     extra_iters=it_ - 1)
            for k in range(K):
                ref = so.istft(o['yf'][k], L, n_fft, n_fft // 2, work_dtype=np.float64)
                errs['out_oracle'] = max(errs.get('out_oracle', 0.0), relerr(f[o_idx][r, k], ref))
                errs['yf_oracle'] = max(errs.get('yf_oracle', 0.0), relerr(f[yf_idx][r, k].T, o['yf'][k]))
    assert errs['out_oracle'] < tol and errs['yf_oracle'] < tol, errs
    return errs


def check_overlapped_halves(make_engine, K=2, M=2, L=6000, n_fft=512, R=3, iters=1, mode=2):
    """Option "overlap_solves" (include/disco_hip.h): the whole-path calls run the batch as two half-batch children, the second on the
    context's side stream.  Rooms are independent and the children keep the launch geometry of the whole batch, so the outputs
    must equal the plain call's BIT FOR BIT; the stage report shows two launches per stage covering R rooms together; nothing is
    allocated by the calls (the children's partial-sum blocks are sized with the context); the option is per context."""
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    plain = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    plain.set_option('overlap_solves', 0)
    over = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft)
    over.set_option('overlap_solves', mode)                   # 2: also for batches far too small to be worth it
    assert plain.get_option('overlap_solves') == 0 and over.get_option('overlap_solves') == mode
    m = plain.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, plain.T, plain.F).numpy()
    over.reserve(1)
    own = over.owned_bytes()
    res = {}
    for name, e in (('plain', plain), ('over', over)):
        e.stage_timing(True)
        if iters > 1:
            out, yf = e.tango_enhance_iterated(y, m, iters=iters)
            z = None
        else:
            out, z, yf = e.tango_enhance(y, m)
        rep = e.stage_report()
        e.stage_timing(False)
        out_enh = e.tango_enhance(y, m, want_z=False, want_yf=False)[0].numpy() if iters == 1 else None
        res[name] = (out.numpy(), None if z is None else z.numpy(), yf.numpy(), out_enh, rep)
    assert over.owned_bytes() == own, (over.owned_bytes(), own)
    for a, b in zip(res['plain'][:4], res['over'][:4]):
        assert (a is None and b is None) or np.array_equal(a, b)
    rp, ro = res['plain'][4], res['over'][4]
    assert set(rp) == set(ro), (set(rp), set(ro))
    for nm in rp:
        assert ro[nm][1] == 2 * rp[nm][1] and ro[nm][2] == rp[nm][2] == rp[nm][1] * R, (nm, rp[nm], ro[nm])
    return {nm: ro[nm][1:] for nm in ro}


def _load_scenes_module(golden_dir):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('make_golden_scenes', os.path.join(golden_dir, 'make_golden_scenes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _per_bin_err(a, b):
    """(F, T) -> (F,) relative l2 error over the frames of every bin."""
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


def check_reference_scene_per_bin(make_engine, golden_dir, idx, staged=False, max_excluded=0.5, tol=1e-4, tol_bin=2e-4):
    """The HIP path against the REFERENCE'S OWN offline_tango on one of the five long scenes of tests/golden/tango_ref_scenes.npz
    (fixed consecutive seeds, 201 frames; make_golden_scenes.py says how they were made and why the comparison is per bin):
      * the (node, bin)s whose dominant-eigenvector sensitivity kappa = cond(Rnn) / (1 - d1/d0) is <= the fixture's cut at BOTH
        steps: z_y and yf of all of them TOGETHER (one signal per node) within `tol` = 1e-4 of the reference's own output, and
        every single one of them within `tol_bin` = 2e-4 (relative l2 over the frames of the bin).  Why 2e-4 per bin: on these
        very bins the reference's own complex64 LAPACK output is up to 9.3e-5 away from the float64 restatement of its own
        algorithm (make_golden_scenes.py prints it) -- a per-bin 1e-4 would test the reference's rounding, not this code;
      * the other bins are counted; their share must stay under `max_excluded`;
      * against the float64 restatement of the reference's algorithm: every KEPT bin within `tol`, ALL bins together (one signal per
        node) within `tol`, and no single bin -- however ill-conditioned -- beyond 2e-3 (float32 spectra perturb a pencil of
        sensitivity 1e5 by that much; the excluded bins are where the reference's complex64 LAPACK is off by up to 2e-2)."""
    import os
    ms = _load_scenes_module(golden_dir)
    g = np.load(os.path.join(golden_dir, 'tango_ref_scenes.npz'))
    K, M, L, seed = int(g[f'sc{idx}_K']), int(g[f'sc{idx}_M']), int(g['L']), int(g[f'sc{idx}_seed'])
    y, s, n = ms.scene(seed, K, M, L)
    assert ms.checksum(y, s, n) == str(g[f'sc{idx}_sha']), 'the regenerated inputs differ from the ones the reference was run on'
    y, s, n = np.stack(y)[None], np.stack(s)[None], np.stack(n)[None]
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L, staged_step2=staged)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F)
    out, z, yf = eng.tango_enhance(y, m)
    z, yf = z.numpy()[0], yf.numpy()[0]
    ok = ms.kappa(g[f'sc{idx}_cond1'], g[f'sc{idx}_gap1'], g[f'sc{idx}_cond2'], g[f'sc{idx}_gap2']) <= float(g['kappa_cut'])
    excluded = float((~ok).mean())
    assert excluded <= max_excluded, excluded
    o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    res = {'excluded': excluded, 'ref_kept': 0.0, 'f64_kept': 0.0, 'f64_signal': 0.0, 'f64_worst_bin': 0.0, 'ref_excluded': 0.0,
           'ref_kept_signal': 0.0}
    for k in range(K):
        for nm, got in (('z_y', z[k].T), ('yf', yf[k].T)):
            ref = g[f'sc{idx}_{nm}{k}']
            e_ref, e_64 = _per_bin_err(got, ref), _per_bin_err(got, o[nm][k])
            res['ref_kept'] = max(res['ref_kept'], float(e_ref[ok[k]].max()))
            res['f64_kept'] = max(res['f64_kept'], float(e_64[ok[k]].max()))
            res['f64_worst_bin'] = max(res['f64_worst_bin'], float(e_64.max()))
            res['f64_signal'] = max(res['f64_signal'], relerr(got, o[nm][k]))
            if (~ok[k]).any():
                res['ref_excluded'] = max(res['ref_excluded'], float(e_ref[~ok[k]].max()))
            res['ref_kept_signal'] = max(res['ref_kept_signal'], relerr(got[ok[k]], ref[ok[k]]))       # all kept bins as one signal
            res['ref_whole_signal'] = max(res.get('ref_whole_signal', 0.0), relerr(got, ref))            # ALL bins, kept or not, as one signal
    assert res['ref_kept'] < tol_bin and res['ref_kept_signal'] < tol, res
    assert res['f64_kept'] < tol and res['f64_signal'] < tol and res['f64_worst_bin'] < 2e-3, res
    # backstop on everything at once: the whole signal, excluded bins included, against the reference's own output.  Documented bound
    # 5e-3: on the excluded bins of these 201-frame scenes the REFERENCE is up to 2e-2 per bin from the exact solution of its own
    # algorithm (make_golden_scenes.py prints it), which is 1-3e-3 of a whole signal; the full-length scenes
    # (check_baseline_shape_reference) have no excluded bins and are held to 1e-4 on the whole signal.
    assert res['ref_whole_signal'] < 5e-3, res
    return res


def _load_baseline_shapes_module(golden_dir):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('make_golden_baseline_shapes', os.path.join(golden_dir, 'make_golden_baseline_shapes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def baseline_shape_inputs(golden_dir, name):
    """Inputs of one BASELINE-shaped scene of tests/golden/tango_ref_baseline_shapes.npz ('c3': 4 x 4, 'c2': 1 x 4; L = 160 000), regenerated
    from the bench's room generator and checked against the SHA-256 the fixture carries -> (g, y, s, n) with [node](M, L) lists."""
    import os
    mb, ms = _load_baseline_shapes_module(golden_dir), _load_scenes_module(golden_dir)
    g = np.load(os.path.join(golden_dir, 'tango_ref_baseline_shapes.npz'))
    y, s, n = mb.inputs(name)
    assert ms.checksum(y, s, n) == str(g[f'{name}_sha']), 'the regenerated inputs differ from the ones the reference was run on'
    return g, y, s, n


def check_baseline_shape_reference(make_engine, golden_dir, name, staged=False, tol=1e-4, tol_bin=2e-4):
    """The HIP path against the REFERENCE'S OWN offline_tango (tango.py:252-457) at BASELINE.json's shape and length: one room of C3
    (4 nodes x 4 mics, L = 160 000, T = 626) or of C2 (1 node x 4 mics), the bench's own synthetic room (make_golden_baseline_shapes.py).
    With 626 frames NO (node, bin) is beyond the sensitivity cut of make_golden_scenes.py (the 201-frame scenes lose 16-49 %), so the
    comparison is on everything: z_y and yf of every node as WHOLE SIGNALS within 1e-4 of the reference's output, every single bin
    within 2e-4 (the reference's own complex64 rounding is part of a per-bin figure), and the same against the float64 restatement.
    Returns the numbers, among them the excluded share (asserted 0) and the whole-signal error against the reference."""
    ms = _load_scenes_module(golden_dir)
    g, y, s, n = baseline_shape_inputs(golden_dir, name)
    K, M, L = int(g[f'{name}_K']), int(g[f'{name}_M']), int(g['L'])
    y, s, n = np.stack(y)[None], np.stack(s)[None], np.stack(n)[None]
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L, staged_step2=staged)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F)
    out, z, yf = eng.tango_enhance(y, m)
    z, yf = z.numpy()[0], yf.numpy()[0]
    ok = ms.kappa(g[f'{name}_cond1'], g[f'{name}_gap1'], g[f'{name}_cond2'], g[f'{name}_gap2']) <= float(g['kappa_cut'])
    res = {'excluded_share': float((~ok).mean()), 'ref_signal': 0.0, 'ref_worst_bin': 0.0, 'f64_signal': 0.0, 'f64_worst_bin': 0.0}
    assert res['excluded_share'] == 0.0, res
    o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    for k in range(K):
        for nm, got in (('z_y', z[k].T), ('yf', yf[k].T)):
            ref = g[f'{name}_{nm}{k}']
            res['ref_signal'] = max(res['ref_signal'], relerr(got, ref))
            res['ref_worst_bin'] = max(res['ref_worst_bin'], float(_per_bin_err(got, ref).max()))
            res['f64_signal'] = max(res['f64_signal'], relerr(got, o[nm][k]))
            res['f64_worst_bin'] = max(res['f64_worst_bin'], float(_per_bin_err(got, o[nm][k]).max()))
    assert res['ref_signal'] < tol and res['ref_worst_bin'] < tol_bin and res['f64_signal'] < tol and res['f64_worst_bin'] < tol_bin, res
    return res


def check_baseline_shape_surface(offline_tango, golden_dir, name, tol=1e-4):
    """The Python call surface (`offline_tango`, the reference's own signature) on a BASELINE-shaped room: the nine outputs' z_y and yf
    as whole signals within 1e-4 of the REFERENCE'S OWN output, no oracle in between, nothing excluded."""
    g, y, s, n = baseline_shape_inputs(golden_dir, name)
    K = int(g[f'{name}_K'])
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mods=[None, None])
    worst = max(relerr(np.asarray(res[i][k]), g[f'{name}_{nm}{k}']) for k in range(K) for i, nm in ((0, 'yf'), (3, 'z_y')))
    assert worst < tol, worst
    return worst


def check_short_reference_scene_per_bin(make_engine, golden_dir, scene, kappa_cut=2e3, tol=1e-4, tol_bin=2e-4):
    """The three short scenes of make_golden.py (17-25 frames) the same way: per (node, bin), against the reference's own output on
    the bins whose sensitivity is <= kappa_cut (2e3: with so few frames the statistics are poorer and the cut is tighter; the
    4 x 4 scene keeps only a few bins); against the float64 restatement on the kept bins and on all bins together (one signal
    per node) -- instead of a blanket 1e-2."""
    import os
    ms = _load_scenes_module(golden_dir)
    g = np.load(os.path.join(golden_dir, f'tango_ref_{scene}.npz'))
    c = np.load(os.path.join(golden_dir, 'tango_ref_short_cond.npz'))
    K = int(g['K'])
    y = np.stack([g[f'y{k}'] for k in range(K)])[None]
    s = np.stack([g[f's{k}'] for k in range(K)])[None]
    n = np.stack([g[f'n{k}'] for k in range(K)])[None]
    R, K, M, L = y.shape
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L)
    m = eng.mask_oracle(s[0, :, 0], n[0, :, 0]).reshape(1, K, eng.T, eng.F)
    out, z, yf = eng.tango_enhance(y, m)
    z, yf = z.numpy()[0], yf.numpy()[0]
    ok = ms.kappa(c[f'{scene}_cond1'], c[f'{scene}_gap1'], c[f'{scene}_cond2'], c[f'{scene}_gap2']) <= kappa_cut
    assert ok.any()
    o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    res = {'kept': float(ok.mean()), 'ref_kept': 0.0, 'f64_kept': 0.0, 'f64_signal': 0.0, 'f64_worst_bin': 0.0}
    for k in range(K):
        assert np.abs(m.numpy()[0, k].T - g[f'masks_z{k}']).max() < 1e-3
        for nm, got in (('z_y', z[k].T), ('yf', yf[k].T)):
            e_ref, e_64 = _per_bin_err(got, g[f'{nm}{k}']), _per_bin_err(got, o[nm][k])
            if ok[k].any():
                res['ref_kept'] = max(res['ref_kept'], float(e_ref[ok[k]].max()))
                res['f64_kept'] = max(res['f64_kept'], float(e_64[ok[k]].max()))
            res['f64_worst_bin'] = max(res['f64_worst_bin'], float(e_64.max()))
            res['f64_signal'] = max(res['f64_signal'], relerr(got, o[nm][k]))
    assert res['ref_kept'] < tol_bin and res['f64_kept'] < tol and res['f64_signal'] < tol and res['f64_worst_bin'] < 2e-3, res
    return res


def check_reference_surface_scene_per_bin(offline_tango, golden_dir, idx, tol=1e-4, tol_bin=2e-4):
    """The Python call surface (`offline_tango`, the reference's own signature) on one long reference-run scene: z_y and yf per
    (node, bin) against the reference's own output on the bins the fixture's sensitivity cut keeps (make_golden_scenes.py)."""
    import os
    ms = _load_scenes_module(golden_dir)
    g = np.load(os.path.join(golden_dir, 'tango_ref_scenes.npz'))
    K, M, L, seed = int(g[f'sc{idx}_K']), int(g[f'sc{idx}_M']), int(g['L']), int(g[f'sc{idx}_seed'])
    y, s, n = ms.scene(seed, K, M, L)
    assert ms.checksum(y, s, n) == str(g[f'sc{idx}_sha'])
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mods=[None, None])
    ok = ms.kappa(g[f'sc{idx}_cond1'], g[f'sc{idx}_gap1'], g[f'sc{idx}_cond2'], g[f'sc{idx}_gap2']) <= float(g['kappa_cut'])
    worst, worst_sig = 0.0, 0.0
    for k in range(K):
        for i, nm in ((0, 'yf'), (3, 'z_y')):
            got, ref = np.asarray(res[i][k]), g[f'sc{idx}_{nm}{k}']
            worst = max(worst, float(_per_bin_err(got, ref)[ok[k]].max()))
            worst_sig = max(worst_sig, relerr(got[ok[k]], ref[ok[k]]))
    assert worst < tol_bin and worst_sig < tol, (worst, worst_sig)         # see check_reference_scene_per_bin for the two bars
    return worst, worst_sig


def check_reference_steps_state(make_engine, K=2, M=2, L=4000):
    """disco_tango_reference(steps = 2) continues from the state a steps = 1 call left in the workspace: same inputs, same
    workspace, nothing in between -- anything else is refused (DISCO_E_ARG) instead of running on whatever the workspace holds
    (include/disco_hip.h; round-2 advice).  steps = 1 then 2 equals steps = 3."""
    from disco_amd import synth
    from disco_amd.engine import DiscoError
    y, s, n = synth.make_rooms_numpy(1, K=K, M=M, L=L)
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L)
    yd, sd, nd = (eng.to_device(a, np.float32)[1] for a in (y, s, n))
    y2 = eng.to_device(y.copy(), np.float32)[1]

    def refused(fn):
        try:
            fn()
        except DiscoError as e:
            assert 'steps = 2' in str(e), e
            return True
        return False
    assert refused(lambda: eng.tango_reference(yd, sd, nd, steps=2))                       # no steps = 1 call at all
    full = {k: v.numpy() for k, v in eng.tango_reference(yd, sd, nd, steps=3).items()}
    assert refused(lambda: eng.tango_reference(yd, sd, nd, steps=2))                       # a steps = 3 call leaves no state to continue
    a = {k: v.numpy() for k, v in eng.tango_reference(yd, sd, nd, steps=1).items()}
    assert refused(lambda: eng.tango_reference(y2, sd, nd, steps=2))                       # other input array
    b = {k: v.numpy() for k, v in eng.tango_reference(yd, sd, nd, steps=2).items()}        # the legitimate continuation
    for k, v in {**a, **b}.items():
        assert np.array_equal(v, full[k]), k
    eng.tango_reference(yd, sd, nd, steps=1)
    m = eng.mask_oracle(s[:, :, 0].reshape(K, L), n[:, :, 0].reshape(K, L)).reshape(1, K, eng.T, eng.F)
    eng.tango_enhance(y, m)                                                                # overwrites the context's own workspace
    assert refused(lambda: eng.tango_reference(yd, sd, nd, steps=2))
    return True


def saturating_masks(rng, K, T, F):
    """Masks over (0.05, 0.95) with whole bins saturated in every frame, as a trained mask estimator produces them (round-5 VERDICT item 2):
    -> mask_z, mask_w (K, T, F) float32 and the bins that carry a saturated statistic."""
    mz = rng.uniform(0.05, 0.95, size=(K, T, F)).astype(np.float32)
    mw = rng.uniform(0.05, 0.95, size=(K, T, F)).astype(np.float32)
    tiny = lambda shape: (1e-5 * rng.uniform(0.1, 1.0, size=shape)).astype(np.float32)
    mz[:, :, 10] = 1.0 - tiny((K, T))              # Rnn ~ 0 in step 1, every node
    mz[1 % K, :, 20] = tiny((T,))                      # Rss ~ 0 in step 1, one node
    mw[:, :, 30] = tiny((K, T))                    # Rss ~ 0 in step 2
    mw[2 % K, :, 40] = 1.0 - tiny((T,))                # Rnn ~ 0 in step 2, one node
    mz[0, :, 50] = 1.0 - tiny((T,))                # both steps of one node
    mw[0, :, 50] = tiny((T,))
    mz[3 % K, :, 60] = 1.0                             # exactly saturated but for every 6th frame
    mz[3 % K, ::6, 60] = 1.0 - tiny((len(range(0, T, 6)),)) * 10
    mw[:, :, 70] = 1.0 - rng.integers(1, 4, size=(K, T)).astype(np.float32) * np.float32(2.0 ** -24)    # (1 - m) is one to three float32 rounding units
    return mz, mw, [10, 20, 30, 40, 50, 60, 70]


def check_saturating_masks(make_engine, K=4, M=4, L=16000, n_fft=512, seed=5):
    """Predicted masks that saturate over whole bins (Rss ~ 0, Rnn ~ 0, both): the whole path through the C ABI, scored the way bench.py
    scores C4 (bench.score_given_masks): the unflagged bins at 1e-4 against the float64 oracle, the flagged bins of every node within
    max(1e-4 of the node's spectrum, twice the distance the reference's own solve keeps from the same oracle there) (complex64 statistics,
    scipy.linalg.eig + eps / 1e6 clamps, internal_formulas.py:56-73), output finite.  Every saturated bin must be among the flagged ones."""
    import os
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    import bench
    from disco_amd import synth
    y, s, n, _ = synth.make_room_numpy(3, K=K, M=M, L=L)
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L, n_fft=n_fft)
    rng = np.random.default_rng(seed)
    mz, mw, bins = saturating_masks(rng, K, eng.T, eng.F)
    out, _, yf = eng.tango_enhance(y[None], mz[None], mw[None], want_z=False, want_yf=True)
    out, yf = out.numpy()[0], yf.numpy()[0]
    assert np.isfinite(out).all() and np.isfinite(yf).all()
    masks = ([np.ascontiguousarray(mz[k].T).astype(np.float64) for k in range(K)], [np.ascontiguousarray(mw[k].T).astype(np.float64) for k in range(K)])
    fb, _ = bench.flagged_bins(masks)
    assert list(fb) == bins, fb
    s0, n0 = np.zeros_like(y), np.zeros_like(y)
    s0[:, 0], n0[:, 0] = s[:, 0], n[:, 0]
    e, info = bench.score_given_masks(y, s0, n0, out, masks, yf, n_fft)
    assert e < 1e-4 and info['flagged_by_weight'] == len(bins) <= info['flagged_bins'] and info['unflagged_rel'] < 1e-4 and info['flagged_ratio'] <= 1.0, info
    assert info['spectra_vs_timed_output'] < 1e-5, info
    return e, info


# ---- the image-source generator, pinned where it can be without pyroomacoustics (round-5 VERDICT item 8) -------------------------------
def ism_hand_case():
    """A shoebox whose direct path and six first-order images can be written down by hand (mirror the source in each wall): room 6.5 x 4 x 4 m,
    source (1, 2, 2), microphone (4, 2, 2), c = 320 m/s at 16 kHz = 50 samples per metre, absorption 0.36 (amplitude 0.8 per reflection).
      direct                      (1, 2, 2)            d = 3 m   -> sample 150   amplitude 1 / (4 pi 3)
      wall x = 0                  (-1, 2, 2)           d = 5     -> 250          0.8 / (4 pi 5)
      wall y = 0, y = 4           (1, -2, 2) (1, 6, 2) d = 5 (3-4-5 triangle)
      wall z = 0, z = 4           (1, 2, -2) (1, 2, 6) d = 5
      wall x = 6.5                (12, 2, 2)           d = 8     -> 400          0.8 / (4 pi 8)
    All delays are whole samples, so the fractional-delay filter is a unit impulse (its Hann-windowed sinc is 1 at the centre and 0 at every
    other tap) and the response is exactly three impulses, shifted by the filter's 40-sample centre."""
    dims, src, mic = np.array([6.5, 4.0, 4.0]), np.array([1.0, 2.0, 2.0]), np.array([4.0, 2.0, 2.0])
    want = np.zeros(1024)
    want[150 + 40] = 1.0 / (4 * np.pi * 3.0)
    want[250 + 40] = 5 * 0.8 / (4 * np.pi * 5.0)
    want[400 + 40] = 0.8 / (4 * np.pi * 8.0)
    return dims, 0.36, src, mic, 320.0, want


def ism_images_by_mirroring(dims, src, max_order):
    """{image position: fewest reflections that reach it}: the source mirrored in the six walls, again and again -- the geometric
    construction itself, not the lattice formula the generator uses."""
    src = np.asarray(src, np.float64)
    seen = {tuple(np.round(src, 7))}
    level = {tuple(src): 0}                    # exact position -> order (the rounded copy only recognises a point reached twice)
    frontier = [src]
    for order in range(1, max_order + 1):
        nxt = []
        for p in frontier:
            for ax in range(3):
                for wall in (0.0, dims[ax]):
                    q = p.copy()
                    q[ax] = 2.0 * wall - p[ax]
                    key = tuple(np.round(q, 7))
                    if key not in seen:
                        seen.add(key)
                        level[tuple(q)] = order
                        nxt.append(q)
        frontier = nxt
    return level


def ism_render(images, absorption, mic, fs, c_sound, Lh):
    """Images -> response by the package's documented rendering (sqrt(1 - absorption) per reflection, 1 / (4 pi d), 81-tap Hann-windowed sinc
    centred 40 samples late), written as a plain loop."""
    h = np.zeros(Lh)
    win = np.hanning(81)
    for pos, order in images.items():
        d = float(np.linalg.norm(np.asarray(pos) - mic))
        tau = d / c_sound * fs
        ip = int(np.floor(tau))
        if ip >= Lh:
            continue
        for k in range(-40, 41):
            i = ip + k + 40
            if 0 <= i < Lh:
                h[i] += (1.0 - absorption) ** (0.5 * order) / (4 * np.pi * d) * win[k + 40] * np.sinc(k - (tau - ip))
    return h


def schroeder_rt60(h, fs=16000.0, lo=-5.0, hi=-25.0):
    e = np.cumsum(h[::-1] ** 2)[::-1]
    e = 10 * np.log10(np.maximum(e / e[0], 1e-30))
    i0, i1 = int(np.argmax(e <= lo)), int(np.argmax(e <= hi))
    slope = np.polyfit(np.arange(i0, i1) / fs, e[i0:i1], 1)[0]
    return -60.0 / slope


def check_ism_pinned(rir_fn, tol=2e-5):
    """rir_fn(dims (3,), absorption, src (3,), mic (3,), max_order, c_sound, rir_len) -> (rir_len,) response.  What holds without
    pyroomacoustics at hand (convolve_signals.py:243-246, 94-95): (1) the hand-derived order-1 case; (2) images of order <= 3 against the
    mirror construction; (3) reciprocity at the reference's order 20; (4) sqrt(1 - absorption) per reflection: the order-2 response is a
    quadratic in that factor; (5) the decay against the relation the reference itself draws its absorption from (room_setups.py:92, Eyring):
    a specular shoebox decays slower than the diffuse-field value, by 1.3 ... 1.7 in these rooms -- asserted within [1.1, 1.9], and
    monotone in the absorption."""
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    out = {}
    dims, ab, src, mic, c, want = ism_hand_case()
    out['hand_order1'] = rel(rir_fn(dims, ab, src, mic, 1, c, 1024), want)
    assert out['hand_order1'] < tol, out
    rng = np.random.default_rng(7)
    dims = np.array([rng.uniform(3, 8), rng.uniform(3, 5), rng.uniform(2.5, 3)])
    src, mic = rng.uniform(0.2, 0.8, 3) * dims, rng.uniform(0.2, 0.8, 3) * dims
    imgs = ism_images_by_mirroring(dims, src, 3)
    assert len(imgs) == 63                                   # 1 + 6 + 18 + 38 lattice points of L1 norm <= 3
    out['mirror_order3'] = rel(rir_fn(dims, 0.3, src, mic, 3, 343.0, 2048), ism_render(imgs, 0.3, mic, 16000.0, 343.0, 2048))
    assert out['mirror_order3'] < tol, out
    a, b = rir_fn(dims, 0.3, src, mic, 20, 343.0, 4096), rir_fn(dims, 0.3, mic, src, 20, 343.0, 4096)
    out['reciprocity_order20'] = rel(a, b)
    assert out['reciprocity_order20'] < tol, out
    g = np.array([0.5, 0.8, 1.0])
    hs = np.stack([rir_fn(dims, 1.0 - gi * gi, src, mic, 2, 343.0, 2048) for gi in g])
    coef = np.linalg.solve(np.vander(g, 3, increasing=True), hs)              # h = h0 + g h1 + g^2 h2
    parts = [ism_render({p: 0 for p, o in ism_images_by_mirroring(dims, src, 2).items() if o == k}, 0.0, mic, 16000.0, 343.0, 2048) for k in range(3)]
    out['per_reflection_gain'] = max(rel(coef[k], parts[k]) for k in range(3))
    assert out['per_reflection_gain'] < 20 * tol, out
    ratios, rts = [], []
    for alpha in (0.45, 0.6):
        vol, sur = dims.prod(), 2 * (dims[0] * dims[1] + dims[0] * dims[2] + dims[1] * dims[2])
        eyring = 0.1611 * vol / (-sur * np.log(1.0 - alpha))                  # room_setups.py:92 solved for beta (its 1.7e-5 air term dropped)
        rt = schroeder_rt60(rir_fn(dims, alpha, src, mic, 20, 343.0, 8192))
        ratios.append(rt / eyring)
        rts.append(rt)
    out['rt60_over_eyring'] = ratios
    assert all(1.1 < r_ < 1.9 for r_ in ratios) and rts[1] < rts[0], out
    return out


def check_ism_pinned_hip(make_engine, tol=2e-5):
    """check_ism_pinned on disco_ism_rir (float32 positions and delays: 2e-5 of the largest tap)."""
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)

    def rir(dims, ab, src, mic, order, c, Lh):
        f32 = lambda a: np.asarray(a, np.float32)
        return eng.ism_rir(f32(dims)[None], f32([ab]), f32(src)[None, None], f32(mic)[None, None], max_order=order, c_sound=c,
                           rir_len=Lh).numpy()[0, 0, 0].astype(np.float64)
    return check_ism_pinned(rir, tol=tol)


def check_conv3x3_pool4(lib, device, shapes=((3, 1, 32, 30, 257), (2, 4, 32, 19, 257), (2, 8, 32, 11, 257), (1, 3, 64, 12, 130), (2, 2, 16, 7, 64))):
    """disco_conv3x3_pool4 (the CRNN's first block in one pass: 3x3 convolution with padding (0, 1), bias, MaxPool (1, 4) floor mode) against
    torch's conv2d + max_pool2d in float64 on the same values; (B, C_in, C_out, T_in, F) per case, incl. bins the pooling drops, a last
    workgroup with fewer frames than its tile, and NaN propagation like torch.nn.MaxPool2d.  Shapes outside the direct form are refused."""
    import torch
    errs = []
    for (B, Ci, Co, T, F) in shapes:
        g = torch.Generator().manual_seed(B * 1000 + Ci * 100 + T)
        x = torch.randn((B, Ci, T, F), generator=g)
        w = torch.randn((Co, Ci, 3, 3), generator=g) * 0.3
        b = torch.randn((Co,), generator=g)
        want = torch.nn.functional.max_pool2d(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=(0, 1)), (1, 4)).float()
        xd, wd, bd = x.to(device).contiguous(), w.to(device).contiguous(), b.to(device).contiguous()
        out = torch.empty((B, Co, T - 2, F // 4), dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream().cuda_stream if xd.is_cuda else None
        rc = lib.disco_conv3x3_pool4(None, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), B, Ci, Co, T, F, out.data_ptr(), stream)
        assert rc == 0, (rc, (B, Ci, Co, T, F))
        if xd.is_cuda:
            torch.cuda.synchronize()
        e = float((out.cpu() - want).abs().max() / want.abs().max())
        errs.append(e)
        assert e < 2e-6, ((B, Ci, Co, T, F), e)
    # NaN in one input sample reaches exactly the outputs whose window holds it
    x = torch.zeros((1, 1, 5, 257))
    x[0, 0, 2, 100] = float('nan')
    w, b = torch.ones((32, 1, 3, 3)), torch.zeros(32)
    out = torch.empty((1, 32, 3, 64), dtype=torch.float32, device=device)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    assert lib.disco_conv3x3_pool4(None, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1, 1, 32, 5, 257, out.data_ptr(), None) == 0
    if xd.is_cuda:
        torch.cuda.synchronize()
    nan = torch.isnan(out.cpu())
    want_nan = torch.isnan(torch.nn.functional.max_pool2d(torch.nn.functional.conv2d(x, w, b, padding=(0, 1)), (1, 4)))
    assert torch.equal(nan, want_nan) and int(nan.sum()) == 32 * 3 * 2
    # windows of candidates that are not plain numbers (centre tap only, 2 x +-3e38 inputs): +inf and -inf in one window -> +inf;
    # finite candidates whose sum overflows both ways -> the largest (the zero taps see only finite inputs: no 0 x inf)
    x = torch.zeros((1, 1, 5, 257))
    big_ = 3e38
    x[0, 0, 1, 0:4] = torch.tensor([big_, -big_, 0.0, 0.0])                 # x 2: +inf, -inf
    x[0, 0, 2, 8:12] = torch.tensor([big_, big_, -big_, -big_]) * 0.5        # x 2: +-3e38, finite
    x[0, 0, 2, 12:16] = torch.tensor([-big_, -big_, big_, big_]) * 0.5
    w = torch.zeros((32, 1, 3, 3))
    w[:, 0, 1, 1] = 2.0
    b = torch.linspace(-1, 1, 32)
    out = torch.empty((1, 32, 3, 64), dtype=torch.float32, device=device)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    assert lib.disco_conv3x3_pool4(None, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1, 1, 32, 5, 257, out.data_ptr(), None) == 0
    if xd.is_cuda:
        torch.cuda.synchronize()
    got = out.cpu()
    want = torch.nn.functional.max_pool2d(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=(0, 1)), (1, 4)).float()
    assert not bool(torch.isnan(want).any()) and not bool(torch.isnan(got).any()), torch.nonzero(torch.isnan(got))[:8]
    assert torch.equal(got, want), torch.nonzero(got != want)[:8]
    assert bool((got[0, :, 0, 0] == float('inf')).all()) and bool((got[0, :, 1, 2:4] == want[0, :, 1, 2:4]).all()) and bool(torch.isfinite(got[0, :, 1, 2:4]).all())
    # refused, not mis-computed
    assert lib.disco_conv3x3_pool4(None, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1, 32, 64, 5, 64, out.data_ptr(), None) == -2      # 32 input channels
    assert lib.disco_conv3x3_pool4(None, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1, 1, 32, 5, 513, out.data_ptr(), None) == -2      # 513 bins
    assert lib.disco_conv3x3_pool4(None, None, wd.data_ptr(), bd.data_ptr(), 1, 1, 32, 5, 257, out.data_ptr(), None) == -1
    return errs


def check_crnn_features(lib, device, R=2, K=3, M=2, T=9, F=17):
    """disco_crnn_features against the operations it replaces (tango.py:338, 391; get_z_for_mask 'zs_hat', :158-186; prepare_data's clip then
    pad, speech_enhancement/utils.py:69-138): |X[..., mic]| and the other nodes' |z| in node order, clipped to [1e-6, 1e3], zero rows before
    and after; the step-1 form (no z) and the step-2 form."""
    import torch
    from disco_amd.dnn.crnn import STFT_MAX, STFT_MIN, get_z_for_mask
    g = torch.Generator().manual_seed(3)
    X = torch.view_as_complex(torch.randn((R, K, T, F, M, 2), generator=g)).contiguous()
    z = torch.view_as_complex(torch.randn((R, K, T, F, 2), generator=g)).contiguous()
    X[0, 0, 0, 0, :] = 1e-9                                   # below the clip
    X[0, 1, 2, 3, :] = 5e3                                    # above it
    errs = []
    for with_z, mic, pad in ((False, 1, (10, 10)), (True, 0, (10, 10)), (True, 0, (17, 3))):
        C_ = K if with_z else 1
        Tp = pad[0] + T + pad[1]
        Xd, zd = X.to(device), z.to(device)
        out = torch.empty((R * K, C_, Tp, F), dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream().cuda_stream if Xd.is_cuda else None
        rc = lib.disco_crnn_features(None, Xd.data_ptr(), zd.data_ptr() if with_z else None, R, K, M, T, F, mic, pad[0], pad[1], STFT_MIN, STFT_MAX,
                                     out.data_ptr(), stream)
        assert rc == 0, rc
        if Xd.is_cuda:
            torch.cuda.synchronize()
        want = torch.zeros((R, K, C_, Tp, F))
        want[:, :, 0, pad[0]:pad[0] + T] = X[..., mic].abs()
        if with_z:
            zmag = z.abs()
            for k in range(K):
                want[:, k, 1:, pad[0]:pad[0] + T] = get_z_for_mask(zmag.transpose(0, 1), None, k, K, 'zs_hat').transpose(0, 1)
        want[:, :, :, pad[0]:pad[0] + T] = want[:, :, :, pad[0]:pad[0] + T].clamp(STFT_MIN, STFT_MAX)
        got = out.cpu().view(R, K, C_, Tp, F)
        e = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
        assert e < 3e-7 and float(got[:, :, :, :pad[0]].abs().max()) == 0.0 and float(got[:, :, :, pad[0] + T:].abs().max()) == 0.0, e
        assert float(got[0, 0, 0, pad[0], 0]) == float(torch.tensor(STFT_MIN, dtype=torch.float32)) if mic < M else True
        errs.append(e)
    # NaN passes the clip, as np.clip / torch.clamp leave it (a NaN spectrum must not turn into silence); +-inf clips to hi.  X's NaN sits
    # on microphone 0 only, z's reaches the other nodes' channels
    Xn, zn = X.clone(), z.clone()
    Xn[1, 2, 4, 5, 0] = complex(float('nan'), 0.5)
    Xn[0, 1, 6, 9, :] = complex(float('inf'), 1.0)
    Xn[1, 0, 7, 2, :] = complex(-1.0, float('-inf'))
    zn[1, 0, 3, 7] = complex(float('nan'), -2.0)
    zn[0, 2, 2, 2] = complex(float('-inf'), 0.0)
    for mic in (0, 1):
        pad = (10, 10)
        Tp = pad[0] + T + pad[1]
        Xd, zd = Xn.to(device), zn.to(device)
        out = torch.empty((R * K, K, Tp, F), dtype=torch.float32, device=device)
        assert lib.disco_crnn_features(None, Xd.data_ptr(), zd.data_ptr(), R, K, M, T, F, mic, pad[0], pad[1], STFT_MIN, STFT_MAX, out.data_ptr(),
                                       _stream(Xd)) == 0
        _sync(Xd)
        got = out.cpu().view(R, K, K, Tp, F)[:, :, :, pad[0]:pad[0] + T]
        want = torch.empty((R, K, K, T, F))
        want[:, :, 0] = Xn[..., mic].abs()
        for k in range(K):
            want[:, k, 1:] = get_z_for_mask(zn.abs().transpose(0, 1), None, k, K, 'zs_hat').transpose(0, 1)
        want = want.clamp(STFT_MIN, STFT_MAX)
        nan = torch.isnan(want)
        assert int(nan.sum()) == (K - 1) + (mic == 0), int(nan.sum())
        assert torch.equal(torch.isnan(got), nan), torch.nonzero(torch.isnan(got) != nan).tolist()
        assert float(got[0, 1, 0, 6, 9]) == float(got[1, 0, 0, 7, 2]) == float(torch.tensor(STFT_MAX)) == float(got[0, 0, 2, 2, 2])
        e = float(((got - want).abs() / want.abs().clamp_min(1e-30))[~nan].max())
        assert e < 3e-7, e
        errs.append(e)
    assert lib.disco_crnn_features(None, None, None, R, K, M, T, F, 0, 1, 1, 0.0, 1.0, out.data_ptr(), None) == -1
    assert lib.disco_crnn_features(None, Xd.data_ptr(), None, R, K, M, T, F, M, 1, 1, 0.0, 1.0, out.data_ptr(), None) == -1       # microphone out of range
    return errs


def _sync(t):
    import torch
    if t.is_cuda:
        torch.cuda.synchronize()


def _stream(t):
    import torch
    return torch.cuda.current_stream().cuda_stream if t.is_cuda else None


def _assert_same_floats(got, want, what):
    """Bit-level agreement of two float tensors of one shape: NaN at the same places, every other value equal (inf included)."""
    import torch
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, 'NaN at', torch.nonzero(gn != wn)[:8].tolist())
    bad = (got != want) & ~wn
    assert not bool(bad.any()), (what, 'differs at', torch.nonzero(bad)[:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())


def _gru_gates_ref(gi, gh, h, H):
    """One GRU step's gate arithmetic in float64 (torch.nn.GRU's definition): gi (n, 3H), gh (n, 3H) or (3H,), h (n, H) or None."""
    gi, gh = gi.double(), gh.double()
    gh = gh.expand(gi.shape[0], -1)
    r = 1.0 / (1.0 + (-(gi[:, :H] + gh[:, :H])).exp())
    z = 1.0 / (1.0 + (-(gi[:, H:2 * H] + gh[:, H:2 * H])).exp())
    n = (gi[:, 2 * H:] + r * gh[:, 2 * H:]).tanh()
    return (1 - z) * n + (0 if h is None else z * h.double())


def check_gru_gates(lib, device, cases=((301, 1), (37, 19), (5, 256)), chain=(64, 24, 32), big=False, tol=1e-6, chain_tol=5e-6):
    """disco_gru_gates (the pointwise half of predict_masks' GRU step) against the float64 gate arithmetic, for every (n, H) of `cases`:
    the first step (gh NULL with gh_bias, h_prev NULL), gh without h_prev, the full step with gi a time slice of an [n][steps][3H] tensor
    and with gi rows padded with NaN beyond 3H (never read), h_out aliasing h_prev (bit-identical to the separate buffer), saturating
    pre-activations (+-1e30, +-inf in gi) with a finite answer, and a NaN that must reach exactly its own output.  Then the chained
    form of predict_masks -- one input GEMM, a recurrent GEMM + disco_gru_gates per step -- against torch.nn.GRU in float64 over 8
    and 15 steps (chain = (n, input size, H)): pins the gate order and where the biases go.  big: n = 70 000, H = 256, more elements
    than one launch covers, with pre-activations N(0, 4): float32 evaluation of the tanh argument gi_n + r gh_n errs by about
    2^-23 (|gi_n| + |gh_n|) where the two cancel, and 17.9 M draws of N(0, 16) find such a pair (1.05e-6 under the emulator).
    Returns the largest errors seen."""
    import torch
    errs = {}

    def call(gi, gh, bias, h, out, n, H):
        rc = lib.disco_gru_gates(None, gi.data_ptr(), gi.stride(0), None if gh is None else gh.data_ptr(), None if bias is None else bias.data_ptr(),
                                 None if h is None else h.data_ptr(), out.data_ptr(), n, H, _stream(out))
        assert rc == 0, (rc, n, H)
        _sync(out)
        return out

    def err(name, got, want):
        e = float((got.double().cpu() - want.cpu()).abs().max())
        errs[name] = max(errs.get(name, 0.0), e)
        assert e < tol, (name, e)

    for n, H in cases:
        g = torch.Generator().manual_seed(n * 1000 + H)
        S, st = 8, 5
        gi_all = (torch.randn((n, S, 3 * H), generator=g) * 4).to(device)              # pre-activations ~ N(0, 16)
        gi = gi_all[:, st]                                                                # rows at stride S * 3H
        gh = (torch.randn((n, 3 * H), generator=g) * 4).to(device)
        bias = torch.randn((3 * H,), generator=g).to(device)
        h = (torch.rand((n, H), generator=g) * 2 - 1).to(device)
        out = torch.empty((n, H), device=device)
        err('first_step', call(gi, None, bias, None, out, n, H), _gru_gates_ref(gi, bias, None, H))
        err('no_h_prev', call(gi, gh, None, None, out, n, H), _gru_gates_ref(gi, gh, None, H))
        err('full_step', call(gi, gh, None, h, out, n, H), _gru_gates_ref(gi, gh, h, H))
        want = out.clone()
        padded = torch.full((n, 3 * H + 5), float('nan'), device=device)                 # NaN beyond 3H: a stray read shows
        padded[:, :3 * H] = gi
        _assert_same_floats(call(padded, gh, None, h, out, n, H), want, ('padded gi', n, H))
        h2 = h.clone()
        _assert_same_floats(call(gi, gh, None, h2, h2, n, H), want, ('h_out aliasing h_prev', n, H))
        # saturating and infinite pre-activations (the float64 answer is finite), then one NaN per gate in gi
        gi_s, gh_s = gi.clone(), gh.clone()
        k = min(n * H, 6)
        rows, cols = torch.arange(k, device=device) % n, torch.arange(k, device=device) % H
        for part, vals in ((0, (1e30, -1e30, float('inf'), float('-inf'), 1e30, float('-inf'))),
                           (1, (float('-inf'), 1e30, -1e30, float('inf'), float('inf'), -1e30)),
                           (2, (1e30, float('inf'), float('-inf'), -1e30, float('-inf'), 1e30))):
            gi_s[rows, part * H + cols] = torch.tensor(vals[:k], device=device)
        gh_s[rows[::2], 2 * H + cols[::2]] = -1e30
        want_s = _gru_gates_ref(gi_s, gh_s, h, H)
        assert bool(torch.isfinite(want_s).all())
        err('saturating', call(gi_s, gh_s, None, h, out, n, H), want_s)
        err('saturating_first_step', call(gi_s, None, bias, None, out, n, H), _gru_gates_ref(gi_s, bias, None, H))
        gi_n = gi.clone()
        nan_at = [(0, 0), ((n - 1), H + (H - 1)), (n // 2, 2 * H + H // 2)]
        for r_, c_ in nan_at:
            gi_n[r_, c_] = float('nan')
        got = call(gi_n, gh, None, h, out, n, H).cpu()
        want_nan = torch.zeros((n, H), dtype=torch.bool)
        for r_, c_ in nan_at:
            want_nan[r_, c_ % H] = True
        assert torch.equal(torch.isnan(got), want_nan), ('NaN', n, H, torch.nonzero(torch.isnan(got)).tolist())
        err('nan_elsewhere', got[~want_nan], _gru_gates_ref(gi, gh, h, H).cpu()[~want_nan])

    # the recurrence as predict_masks runs it, against torch.nn.GRU (float64, same weights)
    n, I, H = chain
    for S in (8, 15):
        torch.manual_seed(S)
        gru = torch.nn.GRU(I, H, batch_first=True).double()
        x = torch.randn((n, S, I), dtype=torch.float64)
        with torch.no_grad():
            want = gru(x)[0][:, -1]
        w_ih, w_hh, b_ih, b_hh = (p.detach().float().to(device) for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0))
        gi = torch.addmm(b_ih, x.float().to(device).reshape(-1, I), w_ih.t()).view(n, S, 3 * H)
        h = None
        for st in range(S):
            gh = None if h is None else torch.addmm(b_hh, h, w_hh.t())
            h = call(gi[:, st], gh, b_hh if gh is None else None, h, torch.empty((n, H), device=device), n, H)
        e = float((h.double().cpu() - want).abs().max())
        errs[f'chain_{S}'] = e
        assert e < chain_tol, (S, e)

    if big:
        n, H = 70000, 256
        g = torch.Generator(device=device).manual_seed(5)
        gi = torch.randn((n, 3 * H), device=device, generator=g) * 2
        gh = torch.randn((n, 3 * H), device=device, generator=g) * 2
        h = torch.rand((n, H), device=device, generator=g) * 2 - 1
        out = torch.empty((n, H), device=device)
        e = float((call(gi, gh, None, h, out, n, H).double() - _gru_gates_ref(gi, gh, h, H)).abs().max())
        errs['big'] = e
        assert e < tol, ('big', e)
        del gi, gh, h, out

    # refused, not mis-computed
    gi, out, bias = torch.zeros((4, 12), device=device), torch.empty((4, 4), device=device), torch.zeros(12, device=device)
    assert lib.disco_gru_gates(None, gi.data_ptr(), 11, None, bias.data_ptr(), None, out.data_ptr(), 4, 4, None) == -1        # gi_stride < 3H
    assert lib.disco_gru_gates(None, gi.data_ptr(), 12, None, bias.data_ptr(), None, out.data_ptr(), 0, 4, None) == -1        # n < 1
    assert lib.disco_gru_gates(None, gi.data_ptr(), 12, None, bias.data_ptr(), None, out.data_ptr(), 4, 0, None) == -1        # H < 1
    assert lib.disco_gru_gates(None, None, 12, None, bias.data_ptr(), None, out.data_ptr(), 4, 4, None) == -1                  # no gi
    assert lib.disco_gru_gates(None, gi.data_ptr(), 12, None, None, None, out.data_ptr(), 4, 4, None) == -1                    # no gh, no gh_bias
    return errs


def check_maxpool_last4(lib, device, big=False):
    """disco_maxpool_last4 (MaxPool2d((1, 4)) floor mode + per-channel bias) against torch's max_pool2d then + bias in float32: the same
    operations, so equal bit for bit, NaN where torch has NaN.  Row lengths 4, 7, 64, 257 with huge values in the dropped tail, no bias,
    a (B, C, rows) layout whose channel index wraps, and windows whose candidates are non-finite or overflow when summed.  big: more than
    2^28 outputs (the grid-stride loop makes a second pass, as at C4's second block; a 4.3 GB input)."""
    import torch

    def run(x, bias):
        B, C, R, L = x.shape
        out = torch.empty((B, C, R, L // 4), device=x.device)
        rc = lib.disco_maxpool_last4(None, x.data_ptr(), None if bias is None else bias.data_ptr(), B * C * R, L, R, C, out.data_ptr(), _stream(x))
        assert rc == 0, (rc, x.shape)
        _sync(x)
        return out

    def ref(x, bias):
        y = torch.nn.functional.max_pool2d(x, (1, 4))
        return y if bias is None else y + bias.view(1, -1, 1, 1)

    g = torch.Generator().manual_seed(4)
    for shape in ((2, 3, 5, 4), (2, 3, 5, 7), (1, 4, 9, 64), (2, 2, 3, 257), (3, 5, 6, 16)):
        x = torch.randn(shape, generator=g)
        tail = shape[-1] % 4
        if tail:
            x[..., -tail:] = 3e38                              # floor mode drops these: a leak shows as 3e38
        bias = torch.randn((shape[1],), generator=g) * 10      # a different bias per channel
        xd, bd = x.to(device), bias.to(device)
        _assert_same_floats(run(xd, bd), ref(x, bias), ('bias', shape))
        _assert_same_floats(run(xd, None), ref(x, None), ('no bias', shape))
    # windows that are not plain numbers: torch propagates NaN and takes +inf over -inf; a sum of the candidates says NaN for both
    inf, big_ = float('inf'), 3e38
    wins = [[inf, -inf, 0, 0], [big_, big_, -big_, -big_], [-big_, -big_, big_, big_], [float('nan'), 1, 2, 3], [-inf] * 4,
            [1, 2, 3, float('nan')], [-inf, inf, -big_, big_], [0.5, -2, 7, 1]]
    x = torch.tensor(wins, dtype=torch.float32).view(1, 2, 1, 16)
    bias = torch.tensor([0.25, -1.5])
    for b_ in (bias, None):
        got = run(x.to(device), None if b_ is None else b_.to(device))
        _assert_same_floats(got, ref(x, b_), ('non-finite', b_ is not None))
    assert run(x.to(device), None).cpu().view(-1)[:3].tolist() == [inf, float(torch.tensor(big_)), float(torch.tensor(big_))]
    if big:
        B, C, R, L = 409, 64, 642, 64                           # 16.8 M rows of 16 pooled bins: 2^28 + 444 416 outputs
        gd = torch.Generator(device=device).manual_seed(6)
        x = torch.randn((B, C, R, L), device=device, generator=gd)
        x.view(-1)[[0, 5, x.numel() // 2 + 3, x.numel() - 1]] = float('nan')
        x.view(-1)[-8:-4] = torch.tensor([inf, -inf, 0, 0], device=device)
        bias = torch.randn((C,), device=device, generator=gd)
        got = run(x, bias)
        want = ref(x, bias)
        assert got.numel() > 1 << 28
        nan_g, nan_w = torch.isnan(got), torch.isnan(want)
        assert torch.equal(nan_g, nan_w) and int(nan_g.sum()) == 4
        assert bool(((got == want) | nan_w).all())
        del x, got, want, nan_g, nan_w
        torch.cuda.empty_cache()
    # refused, not mis-computed
    x, out, bias = torch.zeros(64, device=device), torch.empty(16, device=device), torch.zeros(2, device=device)
    assert lib.disco_maxpool_last4(None, x.data_ptr(), None, 16, 3, 1, 1, out.data_ptr(), None) == -1                 # row_len < 4
    assert lib.disco_maxpool_last4(None, x.data_ptr(), bias.data_ptr(), 16, 4, 8, 0, out.data_ptr(), None) == -1     # bias, no channels
    return True


def check_crnn_windows(lib, device):
    """disco_crnn_windows against predict_masks' own strided fallback (crnn.py: `as_strided` over (nb, T, c_used, W Fy)), bit for bit:
    n_keep 4, 2048 ('mid': 8 GRU steps x 256) and 3840 (= C W 4, 'last'), a feature map with more frames than T + W - 1, and several
    signals of one channel and one window.  Misaligned or inconsistent arguments are refused."""
    import torch
    W, Fy = 15, 4

    def run(feat, T, n_keep):
        nb, C, Tp, _ = feat.shape
        out = torch.empty((nb * T, n_keep), device=feat.device)
        rc = lib.disco_crnn_windows(None, feat.data_ptr(), nb, C, Tp, T, W, n_keep, out.data_ptr(), _stream(feat))
        assert rc == 0, (rc, feat.shape, T, n_keep)
        _sync(feat)
        return out

    def ref(feat, T, n_keep):
        nb, C, Tp, _ = feat.shape
        c_used = min(C, -(-n_keep // (W * Fy)))
        win = feat.as_strided((nb, T, c_used, W * Fy), (feat.stride(0), Fy, feat.stride(1), 1)).reshape(nb * T, c_used * W * Fy)
        return win[:, :n_keep]

    g = torch.Generator().manual_seed(7)
    for (nb, C, T, extra, n_keep) in ((2, 64, 9, 0, 4), (2, 64, 9, 0, 2048), (2, 64, 9, 0, 3840), (3, 64, 5, 6, 2048), (3, 64, 4, 3, 3840),
                                      (3, 1, 1, 0, 60), (4, 1, 1, 2, 4)):
        feat = torch.randn((nb, C, T + W - 1 + extra, Fy), generator=g)
        _assert_same_floats(run(feat.to(device), T, n_keep), ref(feat, T, n_keep), (nb, C, T, extra, n_keep))
    # refused, not mis-computed
    feat, out = torch.zeros((1, 3, 20, 4), device=device), torch.empty((64, 128), device=device)     # room for a call that is not refused
    f, o = feat.data_ptr(), out.data_ptr()
    assert lib.disco_crnn_windows(None, f, 1, 2, 20, 6, W, 120, o, None) == 0
    _sync(out)
    assert lib.disco_crnn_windows(None, f, 1, 2, 20, 6, W, 6, o, None) == -1            # n_keep % 4
    assert lib.disco_crnn_windows(None, f, 1, 2, 20, 6, W, 124, o, None) == -1          # n_keep > C W 4
    assert lib.disco_crnn_windows(None, f, 1, 2, 20, 7, W, 120, o, None) == -1          # Tp < T + W - 1
    assert lib.disco_crnn_windows(None, f + 4, 1, 2, 19, 5, W, 120, o, None) == -1      # feat off 16-byte alignment
    assert lib.disco_crnn_windows(None, f, 1, 2, 20, 6, W, 120, o + 4, None) == -1      # out off 16-byte alignment
    return True
