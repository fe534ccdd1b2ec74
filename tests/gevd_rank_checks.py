"""Checks of the rank-R GEVD-MWF solve (disco_gevd_mwf, Engine.gevd_mwf, intern_filter(type='gevd', rank=R)).

Shared by tests/test_gpu_gevd_rank.py (real MI355X, `-m gpu`) and tests/test_gevd_rank_emulated.py (the same kernel sources under the
hipemu CPU emulator, small sizes).  `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library under test.

The yardstick is `closed_form`: for a Hermitian pencil with Rnn = L L^H and C = L^-1 Rxx L^-H = V diag(d) V^H,
    w  = L00 L^-H sum_{i < r} f_i v_i conj(v_i[0]),   f_i = dc_i / (dc_i + mu),  dc_i = d_i clamped to [eps, 1e6]  (d descending)
    t1 = L00 L^-H v_0 conj(v_0[0])
which tests/test_gevd_rank_cpu.py pins against the reference's own outputs (tests/golden/intern_filter_rank_ref.npz)."""
import numpy as np

from oracle import mwf_oracle as mo

EPS = 2.220446049250313e-16
ETA = 1e6


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def kept(rank, P):
    """The reference's `D[rank:, :] = 0` keeps this many of P pairs (Python slicing)."""
    return len(range(P)[:int(rank)])


def closed_form(Rxx, Rnn, r, mu=1.0):
    """float64 closed form of intern_filter(type='gevd') keeping the top r pairs; (..., P, P) -> w, t1 (..., P) complex128."""
    Rxx = np.asarray(Rxx, dtype=np.complex128)
    Rnn = np.asarray(Rnn, dtype=np.complex128)
    P = Rxx.shape[-1]
    L = np.linalg.cholesky(Rnn)
    Li = np.linalg.inv(L)
    LiH = np.conjugate(np.swapaxes(Li, -1, -2))
    C = Li @ Rxx @ LiH
    C = 0.5 * (C + np.conjugate(np.swapaxes(C, -1, -2)))
    d, V = np.linalg.eigh(C)
    d, V = d[..., ::-1], V[..., ::-1]                                   # descending
    dc = np.clip(d, EPS, ETA)
    f = dc / (dc + mu)
    f = np.where(np.arange(P) < r, f, 0.0)
    l00 = L[..., 0, 0][..., None]
    u = np.einsum('...ji,...i->...j', V, f * np.conjugate(V[..., 0, :]))   # sum_i f_i conj(V[0, i]) V[:, i]
    w = l00 * np.einsum('...ij,...j->...i', LiH, u)
    u1 = V[..., :, 0] * np.conjugate(V[..., 0, 0])[..., None]
    t1 = l00 * np.einsum('...ij,...j->...i', LiH, u1)
    return w, t1


def pencils(rng, n, P, d):
    """n Hermitian pencils whose generalized eigenvalues are d (descending), built in float64 (d: (P,) or (n, P))."""
    A = rng.standard_normal((n, P, P)) + 1j * rng.standard_normal((n, P, P))
    Rnn = A @ A.conj().transpose(0, 2, 1) / P + 0.5 * np.eye(P)
    L = np.linalg.cholesky(Rnn)
    V, _ = np.linalg.qr(rng.standard_normal((n, P, P)) + 1j * rng.standard_normal((n, P, P)))
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), (n, P))
    C = (V * d[:, None, :]) @ V.conj().transpose(0, 2, 1)
    Rxx = L @ C @ L.conj().transpose(0, 2, 1)
    Rxx = 0.5 * (Rxx + Rxx.conj().transpose(0, 2, 1))
    return Rxx, Rnn


def gapped_spectrum(rng, n, P, ratio=2.5, indefinite=False):
    """(n, P) descending spectra with a ratio >= `ratio` between neighbours (so every truncation boundary is gapped); indefinite:
    the tail is negative."""
    top = 10.0 ** rng.uniform(-0.5, 1.5, (n, 1))
    d = top / ratio ** np.arange(P)[None, :] * rng.uniform(1.0, 1.2, (n, 1))
    if indefinite and P > 1:
        d[:, P // 2:] -= d[:, P // 2 - 1:P // 2] * 1.5
    return d


def ranks_for(P):
    return sorted({0, 1, 2, P // 2, P - 1, P})


def gpu_solve(eng, Rxx, Rnn, r, mu=1.0):
    w, t1 = eng.gevd_mwf(np.ascontiguousarray(Rxx, dtype=np.complex64), np.ascontiguousarray(Rnn, dtype=np.complex64), r, mu=mu)
    return w.numpy(), t1.numpy()


def _err(a, b):
    """per-pencil relative error, worst over the batch (rows of (..., P))"""
    a = np.asarray(a).reshape(-1, np.shape(a)[-1])
    b = np.asarray(b).reshape(-1, np.shape(b)[-1])
    num = np.linalg.norm(a - b, axis=-1)
    den = np.maximum(np.linalg.norm(b, axis=-1), 1e-30)
    return float(np.max(num / den))


def check_sizes(make_engine, sizes=range(1, 17), batches=(1, 37), tol=2e-6, seed=41):
    """Every P, ranks 0, 1, 2, P//2, P-1, P, against the closed form on the SAME complex64 inputs, gapped spectra, mu 1 and 0.3."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for P in sizes:
        for n in batches:
            Rxx, Rnn = pencils(rng, n, P, gapped_spectrum(rng, n, P))
            Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
            for r in ranks_for(P):
                for mu in (1.0, 0.3):
                    w, t1 = gpu_solve(eng, Rxx, Rnn, r, mu)
                    wr, t1r = closed_form(Rxx, Rnn, r, mu)
                    e_t = _err(t1, t1r)
                    e_w = _err(w, wr) if r > 0 else float(np.abs(w).max())
                    assert e_w < tol and e_t < tol, (P, n, r, mu, e_w, e_t)
                    worst = max(worst, e_w, e_t)
    return worst


def check_batch_shapes(make_engine, P, n=100003, tol=2e-6, seed=43):
    """A large ragged batch and a 2-D batch at one P."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    Rxx, Rnn = pencils(rng, n, P, gapped_spectrum(rng, n, P))
    Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
    r = max(P // 2, 1)
    w, t1 = gpu_solve(eng, Rxx, Rnn, r)
    wr, t1r = closed_form(Rxx, Rnn, r)
    e = max(_err(w, wr), _err(t1, t1r))
    assert e < tol, (P, n, e)
    m = 6 * 7
    w2, t12 = gpu_solve(eng, Rxx[:m].reshape(6, 7, P, P), Rnn[:m].reshape(6, 7, P, P), r)
    assert w2.shape == (6, 7, P) and t12.shape == (6, 7, P)
    assert np.array_equal(w2.reshape(m, P), w[:m]) and np.array_equal(t12.reshape(m, P), t1[:m])
    return e


def check_rank1_matches_r1(make_engine, sizes=range(1, 17), n=57, tol=2e-6, seed=47):
    """disco_gevd_mwf(rank=1) against disco_gevd_mwf_r1 on rank-1-plus-noise pencils (check_solver_sizes's construction)."""
    rng = np.random.default_rng(seed)
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
        w, t1 = gpu_solve(eng, Rxx, Rnn, 1)
        w1, t11 = eng.gevd_mwf_r1(Rxx, Rnn, mu=1.0)
        e = max(_err(w, w1.numpy()), _err(t1, t11.numpy()))
        assert e < tol, (P, e)
        worst = max(worst, e)
    return worst


def check_full_rank_no_gap(make_engine, sizes=(1, 2, 3, 4, 5, 7, 8, 9, 15, 16), n=23, tol=2e-6, seed=53):
    """Full rank needs no eigenvalue gap: tiny gaps and exactly repeated eigenvalues; with mu = 0 the result is e1."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for P in sizes:
        for d in (np.full(P, 2.0), 2.0 + 1e-7 * np.arange(P)[::-1], np.repeat([3.0, 0.5], [P - P // 2, P // 2])):
            Rxx, Rnn = pencils(rng, n, P, d)
            Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
            w, t1 = gpu_solve(eng, Rxx, Rnn, P)
            wr, _ = closed_form(Rxx, Rnn, P)
            e = _err(w, wr)
            assert e < tol, (P, d[:2], e)
            w0, _ = gpu_solve(eng, Rxx, Rnn, P + 3, mu=0.0)
            e1 = np.zeros((n, P))
            e1[:, 0] = 1.0
            e0 = float(np.abs(w0 - e1).max())
            assert e0 < tol, (P, e0)
            worst = max(worst, e, e0)
    return worst


def check_degenerate(make_engine, sizes=(1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16), n=29, seed=59):
    """Rxx = 0; singular Rnn (co-rank 1, 2, P - 1); indefinite Rxx (clamped to eps); a NaN pencil inside a batch."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    for P in sizes:
        Rxx, Rnn = pencils(rng, n, P, gapped_spectrum(rng, n, P))
        Rxx, Rnn = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
        # Rxx = 0: w = 0 (every eigenvalue clamps to eps), finite
        w, t1 = gpu_solve(eng, np.zeros_like(Rxx), Rnn, P)
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(t1)) and float(np.abs(w).max()) < 1e-12, P
        # singular Rnn
        for corank in sorted({1, 2, P - 1} - {0}):
            if corank >= P:
                continue
            B = rng.standard_normal((n, P, P - corank)) + 1j * rng.standard_normal((n, P, P - corank))
            Rs = (B @ B.conj().transpose(0, 2, 1)).astype(np.complex64)
            for r in (1, 2, P):
                w, t1 = gpu_solve(eng, Rxx, Rs, r)
                assert np.all(np.isfinite(w)) and np.all(np.isfinite(t1)), (P, corank, r)
                assert float(np.abs(w).max()) < 1e4 and float(np.abs(t1).max()) < 1e4, (P, corank, r)
        # indefinite Rxx = Ryy - Rnn: negative eigenvalues clamp to eps, i.e. those pairs contribute ~0
        d = gapped_spectrum(rng, n, P, indefinite=True)
        Ri, Rn = pencils(rng, n, P, d)
        Ri, Rn = Ri.astype(np.complex64), Rn.astype(np.complex64)
        for r in ranks_for(P):
            w, t1 = gpu_solve(eng, Ri, Rn, r)
            wr, t1r = closed_form(Ri, Rn, r)
            e = max(_err(w, wr) if r > 0 else float(np.abs(w).max()), _err(t1, t1r))
            assert e < 2e-6, (P, r, e)
        # a NaN pencil leaves its neighbours bit-identical
        for r in (0, 1, P):
            w, t1 = gpu_solve(eng, Rxx, Rnn, r)
            Rb = Rxx.copy()
            Rb[n // 2, 0, 0] = np.nan
            wb, t1b = gpu_solve(eng, Rb, Rnn, r)
            keep = np.arange(n) != n // 2
            assert np.array_equal(wb[keep], w[keep]) and np.array_equal(t1b[keep], t1[keep]), (P, r)
            Rb = Rnn.copy()
            Rb[n // 2, P - 1, P - 1] = np.inf
            wb, t1b = gpu_solve(eng, Rxx, Rb, r)
            assert np.array_equal(wb[keep], w[keep]) and np.array_equal(t1b[keep], t1[keep]), (P, r)


def check_singular_corank1_oracle(make_engine, sizes=(2, 3, 4, 5, 7, 9, 15), tol=1e-3, seed=61):
    """Co-rank-1 Rnn (exactly singular in complex64, as check_solver_singular_noise builds it): one infinite generalized eigenvalue,
    clamped to 1e6 by the reference; agrees with the reference restated in float64 (oracle intern_filter, scipy.linalg.eig)."""
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for P in sizes:
        while True:
            # the complex64 rounding can leave the smallest eigenvalue of Rnn just below 0: an indefinite pencil, on which the
            # reference's LAPACK solve and the pivot floor legitimately part ways -- drawn again
            A = rng.standard_normal((P, P - 1)) + 1j * rng.standard_normal((P, P - 1))
            Rnn = (A @ A.conj().T).astype(np.complex64)
            if np.linalg.eigvalsh(Rnn.astype(np.complex128))[0] > 0:
                break
        B = rng.standard_normal((P, P + 2)) + 1j * rng.standard_normal((P, P + 2))
        Rss = (B @ B.conj().T / (P + 2)).astype(np.complex64)
        for r in sorted({1, 2, P}):
            w, t1 = gpu_solve(eng, Rss[None], Rnn[None], r)
            assert np.all(np.isfinite(w)) and float(np.abs(w).max()) < 1e3, (P, r)
            wo, _ = mo.intern_filter(Rss.astype(np.complex128), Rnn.astype(np.complex128), mu=1, type='gevd', rank=r)
            e = relerr(w[0], wo)
            assert e < tol, (P, r, e)
            worst = max(worst, e)
    return worst


def check_against_golden(make_engine, golden, tol_extra=2e-6, tol_abs=2e-4):
    """The reference's own outputs: the kernel's error on the complex64-rounded inputs is at most the closed form's own error from that
    rounding + tol_extra, and under tol_abs."""
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    worst = 0.0
    for c in range(len(golden['case_pencil'])):
        k, a, b = int(golden['case_pencil'][c]), int(golden['case_off'][c]), int(golden['case_off'][c + 1])
        Rxx, Rnn = golden[f'p{k}_Rxx'], golden[f'p{k}_Rnn']
        rank, mu = int(golden['case_rank'][c]), float(golden['case_mu'][c])
        P = Rxx.shape[0]
        r = kept(rank, P)
        if float(mu) == 0.0 and r < P:
            continue
        w_ref, t1_ref = golden['w'][a:b], golden['t1'][a:b]
        R32, N32 = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
        w, t1 = gpu_solve(eng, R32[None], N32[None], r, mu)
        wc, t1c = closed_form(R32.astype(np.complex128), N32.astype(np.complex128), r, mu)
        for got, cf, ref in ((w[0], wc, w_ref), (t1[0], t1c, t1_ref)):
            if np.linalg.norm(ref) < 1e-12:
                assert float(np.abs(got).max()) < 1e-9, (c, P, rank)
                continue
            e, e_cf = relerr(got, ref), relerr(cf, ref)
            assert e <= e_cf + tol_extra and e < tol_abs, (c, P, rank, mu, e, e_cf)
            worst = max(worst, e)
    return worst


def check_surface(make_engine, sizes=(3, 7, 12), tol=2e-6, seed=67):
    """intern_filter(type='gevd', rank=R) and intern_filter_batched(rank=R) through the package (whichever library it is bound to)."""
    from disco_amd.se_utils.internal_formulas import intern_filter, intern_filter_batched
    rng = np.random.default_rng(seed)
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    for P in sizes:
        Rxx, Rnn = pencils(rng, 1, P, gapped_spectrum(rng, 1, P))
        Rxx, Rnn = Rxx[0], Rnn[0]
        R32, N32 = Rxx.astype(np.complex64), Rnn.astype(np.complex64)
        for rank in (2, P, P + 3, 0, -1, -P - 2, np.int64(2), np.int32(P - 1)):
            w, (t1, si) = intern_filter(Rxx, Rnn, mu=0.3, type='gevd', rank=rank)
            assert w.dtype == np.complex128 and t1.dtype == np.complex128 and w.shape == t1.shape == (P,)
            assert si.dtype == np.int64 and np.array_equal(si, np.arange(P))
            r = kept(rank, P)
            wr, t1r = closed_form(R32, N32, r, 0.3)
            assert (relerr(w, wr) if r > 0 else float(np.abs(w).max())) < tol, (P, rank)
            assert relerr(t1, t1r) < tol, (P, rank)
            wo, (t1o, _) = mo.intern_filter(Rxx, Rnn, mu=0.3, type='gevd', rank=int(rank))
            assert (relerr(w, wo) if r > 0 else float(np.abs(w).max())) < 1e-4, (P, rank)
            assert relerr(t1, t1o) < 1e-4, (P, rank)
        # mu = 0: singular inv(D + 0 I) wherever a pair is dropped, as in the reference; full rank gives e1
        for rank in (0, 2, P - 1, -1):
            try:
                intern_filter(Rxx, Rnn, mu=0, type='gevd', rank=rank)
                raise AssertionError(('no LinAlgError', P, rank))
            except np.linalg.LinAlgError:
                pass
        for rank in (P, P + 3):
            w, _ = intern_filter(Rxx, Rnn, mu=0, type='gevd', rank=rank)
            e1 = np.zeros(P)
            e1[0] = 1.0
            assert float(np.abs(w - e1).max()) < tol, (P, rank)
        # rank 1 keeps its own solver, bit for bit
        w, (t1, si) = intern_filter(Rxx, Rnn, mu=1, type='gevd', rank=1)
        w1, t11 = eng.gevd_mwf_r1(R32[None], N32[None], mu=1.0)
        assert np.array_equal(w, w1.numpy()[0].astype(np.complex128)) and np.array_equal(t1, t11.numpy()[0].astype(np.complex128))
        # the batched form
        Rb, Nb = pencils(rng, 6, P, gapped_spectrum(rng, 6, P))
        Rb, Nb = Rb.reshape(2, 3, P, P), Nb.reshape(2, 3, P, P)
        for rank in (2, P, -1):
            wb, t1b = intern_filter_batched(Rb, Nb, mu=0.3, rank=rank)
            assert wb.shape == t1b.shape == (2, 3, P) and wb.dtype == np.complex64
            wr, t1r = closed_form(Rb.astype(np.complex64), Nb.astype(np.complex64), kept(rank, P), 0.3)
            assert _err(wb, wr) < tol and _err(t1b, t1r) < tol, (P, rank)
        wb, t1b = intern_filter_batched(Rb, Nb, mu=0.3)
        w1, t11 = eng.gevd_mwf_r1(Rb.astype(np.complex64), Nb.astype(np.complex64), mu=0.3)
        assert np.array_equal(wb, w1.numpy()) and np.array_equal(t1b, t11.numpy())
