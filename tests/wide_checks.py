"""Checks of the wide-network route: step-2 pencils of 17 <= P = M + K - 1 <= 32 channels (csrc/k_cov_wide.h, csrc/k_solve_wide.h,
k_apply_m<M, 31>).  Shared by tests/test_gpu_wide_network.py (MI355X, `-m gpu`) and tests/test_wide_network_emulated.py (hipemu, toy
sizes); `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library under test.

Also the seeded scene generator of tests/golden/tango_ref_wide.npz: make_golden_wide.py runs the reference's offline_tango on
wide_scene(...) and stores only the seeds, a checksum of the float32 inputs and the reference's outputs; the tests regenerate the inputs."""
import hashlib

import numpy as np

import parity_checks as pc
from oracle import mwf_oracle as mo
from oracle import tango_oracle as to

relerr = pc.relerr

# the three scenes of tango_ref_wide.npz: (name, K, mics per node, seed).  P2 = max M_k + K - 1: 17, 32, 19.
WIDE_SCENES = (
    ('k16m2', 16, (2,) * 16, 101),
    ('k25m8', 25, (8,) * 25, 102),
    ('k12ragged', 12, (2, 3, 4, 5, 6, 7, 8, 2, 3, 4, 5, 6), 103),
)
WIDE_N_FFT = 512


def wide_scene_length(K, mics):
    """samples for T >= 4 P2 + 2 frames (hop 256): Rnn of a scene is never rank-deficient"""
    P2 = max(mics) + K - 1
    return (4 * P2 + 2) * (WIDE_N_FFT // 2)


def wide_scene(K, mics, seed, L=None):
    """lists of K (M_k, L) float32 arrays y, s, n: one point source and diffuse-ish noise seen through random short FIR channels"""
    rng = np.random.default_rng(seed)
    L = L or wide_scene_length(K, mics)
    src = rng.standard_normal(L + 64)
    y, s, n = [], [], []
    for k in range(K):
        M = mics[k]
        h = rng.standard_normal((M, 16)) * np.exp(-np.arange(16) / 4.0)
        sk = np.stack([np.convolve(src, h[m], mode='full')[64:64 + L] for m in range(M)])
        common = rng.standard_normal(L + 8)
        nk = 0.5 * rng.standard_normal((M, L)) + 0.3 * np.stack([common[m % 8:m % 8 + L] for m in range(M)])
        sk = (0.3 * sk).astype(np.float32)
        nk = (0.3 * nk).astype(np.float32)
        s.append(sk)
        n.append(nk)
        y.append((sk + nk).astype(np.float32))
    return y, s, n


def checksum(y, s, n):
    h = hashlib.sha256()
    for part in (y, s, n):
        for a in part:
            h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def _rank1_noise_pencils(rng, n, P):
    T = 6 * P + 5
    a = rng.standard_normal((n, P, 1)) + 1j * rng.standard_normal((n, P, 1))
    X = a * (rng.standard_normal((n, 1, T)) + 1j * rng.standard_normal((n, 1, T))) + 0.3 * (
        rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T)))
    Nn = rng.standard_normal((n, P, T)) + 1j * rng.standard_normal((n, P, T))
    return (X @ X.conj().transpose(0, 2, 1) / T).astype(np.complex64), (Nn @ Nn.conj().transpose(0, 2, 1) / T).astype(np.complex64)


def check_solver_full(make_engine, sizes=range(17, 33), n=37, tol=2e-6, seed=41):
    """full row-major matrices (disco_gevd_mwf_r1) against the float64 closed form; n is odd on purpose (no multiple of anything)"""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = {}
    for P in sizes:
        Rxx, Rnn = _rank1_noise_pencils(rng, n, P)
        w, t1 = eng.gevd_mwf_r1(Rxx, Rnn)
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 1.0)
        e = max(relerr(w.numpy(), wr), relerr(t1.numpy(), t1r))
        assert e < tol, (P, e)
        # mu changes only the gain
        w3, _ = eng.gevd_mwf_r1(Rxx, Rnn, mu=0.3)
        wr3, _, _ = mo.gevd_mwf_r1_hermitian(Rxx, Rnn, 0.3)
        assert relerr(w3.numpy(), wr3) < tol, P
        worst[P] = e
    return worst


def _scene_stft(rng, R, K, M, T, F):
    return pc._rand_stft_scene(rng, R, K, M, T, F)


def check_solver_from_partials(make_engine, K, M, R=1, L=None, tol=2e-6, seed=43):
    """the pending solve straight from the wide covariance kernel's partial sums == the solve of the matrices disco_cov_masked hands out
    (the same sums, combined in float64 and rounded once), and both against the float64 closed form on those matrices"""
    rng = np.random.default_rng(seed)
    P = M + K - 1
    L = L or (4 * P + 3) * 256
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    X, mask = _scene_stft(rng, R, K, M, eng.T, eng.F)
    z = (X[..., 0] * 0.8 + 0.1 * X[..., -1]).astype(np.complex64)
    Rss, Rnn = eng.cov_masked(X, mask, z, z)
    wp, t1p = eng.gevd_mwf_r1_pending(P, want_t1=True)
    w, t1 = eng.gevd_mwf_r1(Rss, Rnn)
    wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rss.numpy(), Rnn.numpy(), 1.0)
    e_full = max(relerr(w.numpy(), wr), relerr(t1.numpy(), t1r))
    # the pending solve reads the UNSCALED sums (rounded once), disco_cov_masked's matrices are the means (rounded after the 1 / T):
    # two roundings of the same statistics.  As check_cov_solve_apply does for its ill-conditioned shapes, the pending answer is held
    # to whichever of the complex64 matrices' and the float64 statistics' closed form is closer, at the bar of that check
    rs, rn = pc.oracle_cov(X, mask, z, z)
    w64, t164, _ = mo.gevd_mwf_r1_hermitian(rs, rn, 1.0)
    e_pend = min(max(relerr(wp.numpy(), wr), relerr(t1p.numpy(), t1r)), max(relerr(wp.numpy(), w64), relerr(t1p.numpy(), t164)))
    # bar of the pending answer: the float32 rounding of the sums (~6e-8 per entry) times the sensitivity of a 32 x 32 pencil of ~4 P
    # frames reaches 7e-6 (K = 25, M = 8); the solver itself is held to `tol` by e_full and check_solver_full
    assert e_full < tol and e_pend < 2e-5, (e_full, e_pend)
    return {'full': e_full, 'pending': e_pend}


def check_solver_small_gap(make_engine, sizes=(17, 24, 32), gaps=(0.5, 0.9, 0.99), n=9, seed=45):
    """close top pair d1 / d0 up to 0.99: bar 2e-6 / (1 - d1/d0), as check_solver_small_gap of parity_checks"""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    out = {}
    for P in sizes:
        for gap in gaps:
            d = np.concatenate([[1.0, gap], np.linspace(0.3 * gap, 0.01, P - 2)])
            A, B = pc._pencil_with_spectrum(rng, n, P, d)
            A, B = A.astype(np.complex64), B.astype(np.complex64)
            w, t1 = eng.gevd_mwf_r1(A, B)
            wr, t1r, _ = mo.gevd_mwf_r1_hermitian(A, B, 1.0)
            e = max(relerr(w.numpy(), wr), relerr(t1.numpy(), t1r))
            assert e < 2e-6 / (1.0 - gap), (P, gap, e)
            out[(P, gap)] = e
    return out


def check_solver_nan_neighbours(make_engine, P=20, n=11, seed=47):
    """a NaN pencil and an inf pencil between finite ones: the finite ones are solved exactly as without them"""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    Rxx, Rnn = _rank1_noise_pencils(rng, n, P)
    w0, t10 = eng.gevd_mwf_r1(Rxx, Rnn)
    A, B = Rxx.copy(), Rnn.copy()
    A[3, 2, 5] = np.nan
    B[7, 0, 0] = np.inf
    w, t1 = eng.gevd_mwf_r1(A, B)
    keep = np.array([i not in (3, 7) for i in range(n)])
    assert np.array_equal(w.numpy()[keep], w0.numpy()[keep]) and np.array_equal(t1.numpy()[keep], t10.numpy()[keep])
    return True


# ---- staged covariance / solve / apply ------------------------------------------------------------------------------------------
def check_staged(make_engine, K, M, R=1, L=None, seed=49):
    """disco_cov_masked (both mask_for_z forms of the remote rows), the solve and disco_apply at P = M + K - 1 > 16 vs float64"""
    P = M + K - 1
    L = L or (4 * P + 3) * 256
    errs = pc.check_cov_solve_apply(make_engine, R=R, K=K, M=M, L=L, seed=seed)
    errs2 = pc.check_cov_solve_apply(make_engine, R=R, K=K, M=M, L=L, seed=seed + 1, same_z=False, mask_remote=False)
    return {'same_z': errs, 'two_z': errs2}


# ---- the whole path ---------------------------------------------------------------------------------------------------------------
def check_end_to_end(make_engine, R, K, M, L, tol=1e-4):
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    return pc.check_tango_end_to_end(make_engine, y, s, n, tol=tol)


def check_reference_outputs_oracle(make_engine, K, M, L, modes=('local', None, 'distant', 'compressed', 'use_oracle_refs',
                                                                 'use_oracle_zs', 'previous'), tol=1e-4):
    """disco_tango_reference: all nine outputs, every mask_for_z mode, vs the float64 oracle"""
    from disco_amd import synth
    y, s, n = synth.make_rooms_numpy(1, K=K, M=M, L=L)
    eng = make_engine(rooms=1, nodes=K, mics=M, length=L)
    out = {}
    for mode in modes:
        got = eng.tango_reference(y, s, n, mask_for_z=mode)
        o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh', mask_for_z=mode)
        e = 0.0
        for key in ('z_y', 'z_s', 'z_n', 'yf', 'sf', 'nf'):
            g = got[key].numpy()[0]
            for k in range(K):
                e = max(e, relerr(g[k].T, o[key][k]))
        out[mode] = e
        assert e < tol, (mode, e)
    return out


def check_intern_filter(P, n=5, seed=51, tol=2e-6):
    """intern_filter(..., 'gevd', rank=1) on the GPU against the float64 closed form"""
    from disco_amd.se_utils import internal_formulas as inf
    rng = np.random.default_rng(seed)
    Rxx, Rnn = _rank1_noise_pencils(rng, n, P)
    for i in range(n):
        w, (t1, _) = inf.intern_filter(Rxx[i], Rnn[i], mu=1, type='gevd', rank=1)
        wr, t1r, _ = mo.gevd_mwf_r1_hermitian(Rxx[i:i + 1], Rnn[i:i + 1], 1.0)
        assert relerr(np.asarray(w), wr[0]) < tol and relerr(np.asarray(t1), t1r[0]) < tol, i
    return True


def check_refusals(make_engine, lib_error):
    """what stays out of scope says so, naming its limit"""
    import pytest
    rng = np.random.default_rng(53)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    A, B = _rank1_noise_pencils(rng, 3, 33)
    with pytest.raises(lib_error, match='32'):
        eng.gevd_mwf_r1(A, B)
    A, B = _rank1_noise_pencils(rng, 3, 17)
    with pytest.raises(lib_error, match='16'):
        eng.gevd_mwf(A, B, rank=2)
    with pytest.raises(lib_error, match='16'):
        eng.mwf_filter(A, B, type='r1-mwf')
    # P2 = 33 through the path: 26 nodes x 8 mics
    eng = make_engine(rooms=1, nodes=26, mics=8, length=4096)
    y = np.zeros((1, 26, 8, 4096), np.float32)
    m = np.full((1, 26, eng.T, eng.F), 0.5, np.float32)
    with pytest.raises(lib_error, match='32'):
        eng.tango_enhance(y, m)
    return True


def check_reference_wide(offline_tango, golden_dir, scene):
    """the Python call surface (offline_tango, the reference's signature; ragged node sizes take the per-node path) on one scene of
    tango_ref_wide.npz against the reference's own outputs, scored per (node, bin) as tests/test_wide_network_cpu.py does"""
    import os
    name, K, mics, seed = scene
    g = np.load(os.path.join(golden_dir, 'tango_ref_wide.npz'))
    y, s, n = wide_scene(K, mics, seed)
    assert checksum(y, s, n) == str(g[f'{name}_sha']), 'the regenerated inputs differ from the ones the reference was run on'
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mods=[None, None])
    out = {}
    for key in g.files:
        for i, nm in ((0, 'yf'), (3, 'z_y')):
            if key.startswith(f'{name}_{nm}'):
                k = int(key[len(f'{name}_{nm}'):])
                kappa = g[f'{name}_kappa2'][k].astype(np.float64)
                got = np.asarray(res[i][k])
                e = pc._per_bin_err(got, g[key])
                ratio = e / np.maximum(2e-4, 10 * 5.96e-8 * kappa)
                well = kappa <= 1e4
                e_sig = relerr(got[well], g[key][well]) if well.any() else 0.0
                out[key] = {'worst_ratio': float(ratio.max()), 'well_signal': float(e_sig)}
                assert ratio.max() <= 1.0 and e_sig < 1e-3, (key, out[key])
    assert out
    return out
