#!/usr/bin/env python3
"""Generate tests/golden/intern_filter_rank_ref.npz by RUNNING THE REFERENCE'S OWN intern_filter (type='gevd', every rank).

Runs only where the reference is present; the test-suite only reads the committed .npz.  Usage:
    python -B tests/golden/make_golden_gevd_rank.py
The reference module is imported from a scratch copy under /tmp, never in place (as make_golden.py does).

Pencils (stored once each, as p{k}_Rxx / p{k}_Rnn), for P in 1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16:
  'gap'    complex128, generalized eigenvalues a ratio >= 2 apart (every truncation boundary gapped), Rnn well conditioned
  'indef'  complex128, Rxx = Ryy - Rnn with a gapped spectrum whose lower half is negative (clamped to eps by the reference)
  'corank' complex128, Rnn of co-rank 1 up to a 1e-3 eigenvalue (still positive definite once rounded to complex64): exactly one
           generalized eigenvalue above 1e6 (2e6, clamped to 1e6 by the reference), the rest gapped
  'c64'    complex64 inputs (the reference then solves in single precision)
Cases (case_pencil, case_rank, case_mu; outputs w, t1 flattened, case i at case_off[i]:case_off[i + 1]): every pencil at every rank in
(0, 1, 2, P//2, P-1, P, P+3, -1) and mu in (1, 0.3), w and t1 as the reference returns them."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = '/root/reference'
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16)
MUS = (1.0, 0.3)


def _load_reference():
    scratch = tempfile.mkdtemp(prefix='disco_ref_')
    shutil.copytree(os.path.join(REF, 'disco_theque'), os.path.join(scratch, 'disco_theque'))
    sys.path.insert(0, scratch)
    from disco_theque.se_utils.internal_formulas import intern_filter          # real reference code
    return intern_filter, scratch


def _pencil(rng, P, d, Rnn=None):
    if Rnn is None:
        A = rng.standard_normal((P, P)) + 1j * rng.standard_normal((P, P))
        Rnn = A @ A.conj().T / P + 0.5 * np.eye(P)
    L = np.linalg.cholesky(Rnn)
    V, _ = np.linalg.qr(rng.standard_normal((P, P)) + 1j * rng.standard_normal((P, P)))
    Rxx = L @ ((V * d) @ V.conj().T) @ L.conj().T
    return 0.5 * (Rxx + Rxx.conj().T), 0.5 * (Rnn + Rnn.conj().T)


def _spectrum(rng, P, ratio=2.5):
    return rng.uniform(5.0, 20.0) / ratio ** np.arange(P) * rng.uniform(1.0, 1.2)


def pencils(rng, P):
    out = []
    out.append(('gap', _pencil(rng, P, _spectrum(rng, P))))
    d = _spectrum(rng, P)
    if P > 1:
        d[P // 2:] -= 1.5 * d[P // 2 - 1]
    Ryy, Rnn = _pencil(rng, P, d + 1.0)                 # generalized eigenvalues of (Ryy, Rnn): d + 1 (> 0 where d > -1)
    out.append(('indef', (Ryy - Rnn, Rnn)))           # (Ryy - Rnn, Rnn): d
    if P > 1:
        # Rnn = L L^H, L = U diag(sqrt(s)), s = (1e-5, O(1) ...); the top generalized eigenvector is L's weak direction e_0, with
        # eigenvalue 2e6 (Rxx stays O(2e3) there), the others a gapped spectrum below it
        U, _ = np.linalg.qr(rng.standard_normal((P, P)) + 1j * rng.standard_normal((P, P)))
        L = U * np.sqrt(np.concatenate([[1e-3], rng.uniform(0.5, 2.0, P - 1)]))[None, :]
        V = np.eye(P, dtype=np.complex128)
        V[1:, 1:], _ = np.linalg.qr(rng.standard_normal((P - 1, P - 1)) + 1j * rng.standard_normal((P - 1, P - 1)))
        d = np.concatenate([[2e6], _spectrum(rng, P - 1, ratio=2.0)])
        Rxx, Rnn = L @ ((V * d) @ V.conj().T) @ L.conj().T, L @ L.conj().T
        out.append(('corank', (0.5 * (Rxx + Rxx.conj().T), 0.5 * (Rnn + Rnn.conj().T))))
    Rxx, Rnn = _pencil(rng, P, _spectrum(rng, P))
    out.append(('c64', (Rxx.astype(np.complex64), Rnn.astype(np.complex64))))
    return out


def main():
    intern_filter, scratch = _load_reference()
    rng = np.random.default_rng(2014)
    data, n_p = {}, 0
    case_pencil, case_rank, case_mu, w_all, t1_all = [], [], [], [], []
    try:
        for P in SIZES:
            for kind, (Rxx, Rnn) in pencils(rng, P):
                data[f'p{n_p}_Rxx'], data[f'p{n_p}_Rnn'], data[f'p{n_p}_kind'] = Rxx, Rnn, np.array(kind)
                for rank in sorted({0, 1, 2, P // 2, P - 1, P, P + 3, -1}):
                    for mu in MUS:
                        w, (t1, _) = intern_filter(Rxx.copy(), Rnn.copy(), mu=mu, type='gevd', rank=rank)
                        case_pencil.append(n_p)
                        case_rank.append(rank)
                        case_mu.append(mu)
                        w_all.append(np.asarray(w, dtype=np.complex128))
                        t1_all.append(np.asarray(t1, dtype=np.complex128))
                n_p += 1
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    # the outputs of case i are w[off[i]:off[i + 1]], t1[...] (complex128; a complex64 case's outputs are widened exactly)
    data['case_pencil'], data['case_rank'], data['case_mu'] = np.array(case_pencil), np.array(case_rank), np.array(case_mu)
    data['case_off'] = np.concatenate([[0], np.cumsum([len(w) for w in w_all])])
    data['w'], data['t1'] = np.concatenate(w_all), np.concatenate(t1_all)
    data['n_pencils'], n_c = np.array(n_p), len(case_pencil)
    out = os.path.join(HERE, 'intern_filter_rank_ref.npz')
    np.savez_compressed(out, **data)
    print(out, n_p, 'pencils', n_c, 'cases', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
