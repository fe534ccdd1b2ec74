"""The packed workspace layout of X on the fused route of disco_tango_enhance (option "packed_x"; csrc/k_stft.h k_stft_cov<.., PACK>,
csrc/k_fused.h k_step2_cov_fused<.., PACK>, k_step2_apply_istft<.., PACK>): rows of F - 1 bins, [R][K][T][F - 1][M], the real Nyquist value
in the imaginary half of the DC slot.  Only addresses change, so everything here is an EQUALITY (np.array_equal: +0 == -0) between the
option's two values, except the one oracle comparison that makes sure DC and Nyquist are really there:

  A  check_route_equal      disco_tango_enhance, packed_x 1 against 0: `out`, and z_y when asked for, on T = 86 frames (more than two
                            40-frame runs of the transform waves, 43 frame pairs = an odd number, L = 256 * 85 so that the second frame of
                            the last pair of a run may lie beyond T), 3 rooms (half-batch children of 1 + 2 rooms), overlapped and not
  B  check_dc_nyquist       inputs whose energy sits in DC and Nyquist (a + b (-1)^n + noise): `out` against the float64 oracle at
                            PARITY_TOL, and equal between the two layouts
  C  check_lengths          per-room lengths (disco_set_lengths): equal `out`, exact zeros beyond every room's clip, from a workspace of NaN
  D  check_kernels          k_stft_cov and k_step2_cov_fused through the test-only entries: packed X unpacked on the host equals the public
                            X on every bin, the covariances (the finished partial sums) and z are bit-identical, and so are the step-2
                            filters solved from the re-used step-1 sums
Shared by tests/test_packed_x_emulated.py (hipemu, CPU) and tests/test_gpu_packed_x.py (MI355X)."""
import numpy as np

from disco_amd import synth
from oracle import stft_oracle as so
from oracle import tango_oracle as to

PARITY_TOL = 1e-4
N_FFT, HOP = 512, 256
L_ROUTE = HOP * 85                    # T = 86
SHAPES = ((4, 4), (2, 2), (3, 3), (2, 1), (5, 4))        # (K, M): even-M float4 copy, odd-M per-bin store, M = 1, P = 8
PACKED_STAGES = ('stft_cov1', 'step2_cov', 'step2_apply_istft')
# B: standard deviation of the noise added to a + b (-1)^n (|a|, |b| in 0.4 .. 1.6).  A constant and an alternating part give the SAME DC
# and Nyquist value in every frame, so the speech and noise statistics of those bins are two multiples of one rank-1 matrix plus whatever
# the noise adds: with little noise the pencil is too ill-conditioned for float32 statistics on either layout.  Distance of the
# packed_x = 0 route from the float64 oracle on the emulator, (K, M) = (4, 4) / (3, 3):
#   noise 0.05: 0.89 / -   0.2: 0.21 / 4.6e-2   0.5: 1.4e-2 / 1.5e-3   1: 8.7e-4 / 2.3e-4   2: 1.1e-4 / 9.9e-6   3: 3.0e-5 / 2.4e-6
#   noise 4:    7.9e-6 / 1.5e-6  -> the level used: PARITY_TOL with a factor 12 to spare (3 is what the check asks for)
# DC and Nyquist of a channel are then still ~ (256 a)^2 against 96 * 2 * 16 per bin from the noise: 20 times any other bin, and a swapped
# or dropped value misses the oracle by orders of magnitude.
DC_NY_NOISE = 4.0


def relerr(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _bits(a):
    """array_equal on floats with -0 mapped to +0 (and so on complex parts)"""
    a = np.ascontiguousarray(a)
    v = a.view(np.float32) if a.dtype == np.complex64 else a
    return v + np.float32(0.0)


def _engine(make_engine, R, K, M, L, packed, overlap=None, tuning=None):
    e = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=N_FFT)
    if tuning is not None:
        e.set_tuning(*tuning)
    if overlap is not None:
        e.set_option('overlap_solves', overlap)
    e.set_option('packed_x', packed)
    assert e.get_option('packed_x') == packed
    return e


def _mask(e, s, n):
    R, K, _, L = s.shape
    return e.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, e.T, e.F).numpy()


def _enhance(e, y, m, want_z, workspace=None, mask_w=None):
    """-> out, z (or None), the set of stages the call ran"""
    e.stage_timing(True)
    out, z, _ = e.tango_enhance(y, m, mask_w=mask_w, want_z=want_z, want_yf=False, workspace=workspace)
    stages = set(e.stage_report())
    e.stage_timing(False)
    return out.numpy(), (z.numpy() if want_z else None), stages


# ---- A ------------------------------------------------------------------------------------------------------------------------------
def check_route_equal(make_engine, K, M, R=3, L=L_ROUTE, runs=((0, False), (2, True)), extras=False):
    """runs: (overlap_solves, z_y asked for) of the calls compared.  extras: also a second mask array in step 2 (no step-1 sums re-used:
    k_step2_cov_fused<.., false, PACK>, with z_y) and a call that asks for yf (X then leaves through the public-layout kernels whatever
    the option says)"""
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    done = []
    m = None
    for overlap, want_z in runs:
        engines = [_engine(make_engine, R, K, M, L, packed, overlap) for packed in (0, 1)]
        assert engines[0].workspace_bytes() == engines[1].workspace_bytes() and engines[0].T == 86
        if m is None:
            m = _mask(engines[0], s, n)
        got = [_enhance(e, y, m, want_z) for e in engines]
        for o, z, stages in got:
            assert set(PACKED_STAGES) <= stages, stages                      # both ran the route the option is about
            assert np.isfinite(o).all() and o.any()
        assert np.array_equal(got[0][0], got[1][0]), ('out differs between the layouts', K, M, overlap, want_z)
        if want_z:
            assert np.array_equal(got[0][1], got[1][1]), ('z_y differs between the layouts', K, M, overlap)
            for col in (0, engines[0].F - 1):                                # the two columns that moved
                assert np.array_equal(got[0][1][..., col], got[1][1][..., col]) and got[1][1][..., col].any(), col
        done.append((overlap, want_z))
    if extras:
        mw = np.ascontiguousarray(np.sqrt(m))
        got = [_enhance(e, y, m, True, mask_w=mw) for e in engines]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), ('two masks', K, M)
        a, b = (e.tango_enhance(y, m) for e in engines)
        for u, v in zip(a, b):
            assert np.array_equal(u.numpy(), v.numpy())
        done.append('extras')
    return done


# ---- B ------------------------------------------------------------------------------------------------------------------------------
def dc_nyquist_rooms(R, K, M, L, noise=DC_NY_NOISE, seed=11):
    """target and noise images a + b (-1)^n + noise with their own a, b per room, node and channel; y = s + n"""
    rng = np.random.default_rng(seed)
    alt = (1.0 - 2.0 * (np.arange(L) % 2)).astype(np.float64)
    img = []
    for _ in range(2):
        a = rng.uniform(0.4, 1.6, (R, K, M, 1)) * rng.choice((-1.0, 1.0), (R, K, M, 1))
        b = rng.uniform(0.4, 1.6, (R, K, M, 1)) * rng.choice((-1.0, 1.0), (R, K, M, 1))
        img.append((a + b * alt + noise * rng.standard_normal((R, K, M, L))).astype(np.float32))
    s, n = img
    return (s + n).astype(np.float32), s, n


def check_dc_nyquist(make_engine, K, M, R=2, L=L_ROUTE, tol=PARITY_TOL, room=1.0):
    """room: the factor by which the packed_x = 0 route must stay below tol (3 where the noise level is being confirmed)"""
    y, s, n = dc_nyquist_rooms(R, K, M, L)
    engines = [_engine(make_engine, R, K, M, L, packed) for packed in (0, 1)]
    m = _mask(engines[0], s, n)
    outs = [_enhance(e, y, m, False)[0] for e in engines]
    worst = [0.0, 0.0]
    for r in range(R):
        o = to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
        for k in range(K):
            ref = so.istft(o['yf'][k], L, work_dtype=np.float64)
            for i in range(2):
                worst[i] = max(worst[i], relerr(outs[i][r, k], ref))
    print(f'DC / Nyquist inputs (K, M) = {(K, M)}, noise {DC_NY_NOISE}: out vs float64 oracle  packed_x=0 {worst[0]:.3g}  packed_x=1 {worst[1]:.3g}')
    assert worst[0] * room < tol, ('the public layout itself misses the oracle on these inputs', worst)
    assert worst[1] < tol, worst
    assert np.array_equal(outs[0], outs[1])
    return worst


# ---- C ------------------------------------------------------------------------------------------------------------------------------
def check_lengths(make_engine, K=4, M=4, L=L_ROUTE, overlap=None):
    lengths = [L, L - HOP * 7 - 13, HOP * 3]
    R = len(lengths)
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    for r, Lr in enumerate(lengths):
        for a in (y, s, n):
            a[r, :, :, Lr:] = np.nan                                         # never read
    outs = []
    for packed in (0, 1):
        e = _engine(make_engine, R, K, M, L, packed, overlap)
        e.set_lengths(lengths)
        m = _mask(e, s, n)
        ws = e.to_device(np.full(e.workspace_bytes(), 0xFF, np.uint8), np.uint8)[1]      # NaN in every frame the route leaves unwritten
        o, _, stages = _enhance(e, y, m, False, workspace=ws)
        assert set(PACKED_STAGES) <= stages, stages
        outs.append(o)
    assert np.isfinite(outs[1]).all()
    for r, Lr in enumerate(lengths):
        assert outs[1][r, :, :Lr].any() and not outs[1][r, :, Lr:].any(), ('exact zeros beyond the clip', r)
    assert np.array_equal(outs[0], outs[1])
    return lengths


# ---- D ------------------------------------------------------------------------------------------------------------------------------
def unpack_x(Xp):
    """packed (R, K, T, F - 1, M) -> public (R, K, T, F, M): slot 0 = (Re X[0], Re X[F - 1])"""
    R, K, T, H, M = Xp.shape
    X = np.zeros((R, K, T, H + 1, M), np.complex64)
    X[..., 1:H, :] = Xp[..., 1:, :]
    X[..., 0, :] = Xp[..., 0, :].real
    X[..., H, :] = Xp[..., 0, :].imag
    return X


def check_kernels(make_engine, K, M, R=2, L=HOP * 45 + 100, tuning=(8, 0, 3, 0)):
    """tuning: 8-frame runs of the transform waves (T = 46: two chunks, the second with empty waves), 3 frame chunks in step 2"""
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    e = _engine(make_engine, R, K, M, L, 1, tuning=tuning)
    lib, T, F, P = e.lib, e.T, e.F, M + K - 1
    m = _mask(e, s, n)
    py, ky = e.to_device(y, np.float32)
    pm, km = e.to_device(m, np.float32)
    # k_stft_cov: public against packed
    X, Rss, Rnn = e.stft_cov_fused(ky, km)
    X, Rss, Rnn = X.numpy(), Rss.numpy(), Rnn.numpy()
    assert np.abs(X[..., 0, :].imag).max() == 0 and np.abs(X[..., F - 1, :].imag).max() == 0      # what the packing rests on
    Xp = e.empty((R, K, T, F - 1, M), np.complex64)
    Rss_p, Rnn_p = (e.empty((R, K, F, M, M), np.complex64) for _ in range(2))
    e._chk(lib.disco_selftest_stft_cov_packed(e.ctx, py, pm, Xp.ptr, Rss_p.ptr, Rnn_p.ptr, e.stream))
    assert np.array_equal(_bits(unpack_x(Xp.numpy())), _bits(X)), 'k_stft_cov: the packed X does not unpack to the public one'
    assert X[..., 0, :].real.any() and X[..., F - 1, :].real.any()
    assert np.array_equal(Rss_p.numpy().view(np.uint32), Rss.view(np.uint32)) and np.array_equal(Rnn_p.numpy().view(np.uint32), Rnn.view(np.uint32))
    # k_step2_cov_fused<.., false>: public against packed, on that X
    rng = np.random.default_rng(5)
    w_loc = (rng.standard_normal((R, K, F, M)) + 1j * rng.standard_normal((R, K, F, M))).astype(np.complex64)
    pw, kw = e.to_device(w_loc, np.complex64)
    S2, N2, z = e.step2_cov_fused(X, km, kw)
    z_p = e.empty((R, K, T, F), np.complex64)
    S2_p, N2_p = (e.empty((R, K, F, P, P), np.complex64) for _ in range(2))
    e._chk(lib.disco_selftest_step2_cov_packed(e.ctx, Xp.ptr, pm, pw, z_p.ptr, S2_p.ptr, N2_p.ptr, 0, e.stream))
    assert np.array_equal(z_p.numpy(), z.numpy()), 'k_step2_cov_fused: z differs'
    assert np.array_equal(S2_p.numpy().view(np.uint32), S2.numpy().view(np.uint32)), 'k_step2_cov_fused: Rss differs'
    assert np.array_equal(N2_p.numpy().view(np.uint32), N2.numpy().view(np.uint32)), 'k_step2_cov_fused: Rnn differs'
    # k_step2_cov_fused<.., true>: the step-1 sums re-used, solved straight from the partial sums
    Xd = e.empty((R, K, T, F, M), np.complex64)
    e.stft_cov_fused(ky, km, X_out=Xd, want_cov=False)
    e.step2_cov_fused_reuse(Xd, km, kw)
    w_pub = e.gevd_mwf_r1_pending(P)[0].numpy()
    e._chk(lib.disco_selftest_stft_cov_packed(e.ctx, py, pm, Xp.ptr, None, None, e.stream))
    z_p = e.empty((R, K, T, F), np.complex64)
    e._chk(lib.disco_selftest_step2_cov_packed(e.ctx, Xp.ptr, pm, pw, z_p.ptr, None, None, 1, e.stream))
    w_pk = e.gevd_mwf_r1_pending(P)[0].numpy()
    assert np.array_equal(w_pk.view(np.uint32), w_pub.view(np.uint32)), 'k_step2_cov_fused<.., true>: the filters differ'
    assert np.array_equal(z_p.numpy(), z.numpy())
    return True


# ---- E: nothing is allocated by a compute call, whichever layout -----------------------------------------------------------------------
def check_no_allocation(make_engine, K=3, M=2, R=3, L=HOP * 20):
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    e = _engine(make_engine, R, K, M, L, 0, overlap=2)
    e.reserve(1)
    own = e.owned_bytes()
    m = _mask(e, s, n)
    for packed in (1, 0, 1):
        e.set_option('packed_x', packed)
        assert e.owned_bytes() == own
        e.tango_enhance(y, m, want_z=False, want_yf=False)
        assert e.owned_bytes() == own
    return own
