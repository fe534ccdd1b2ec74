"""The yardstick of the rank-R GEVD-MWF tests (tests/gevd_rank_checks.py: closed_form) against the reference's own intern_filter
outputs (tests/golden/intern_filter_rank_ref.npz, tests/golden/make_golden_gevd_rank.py) and against the oracle's restatement of it;
and the host-side rules of the public surface that need no GPU."""
import os

import numpy as np
import pytest

import gevd_rank_checks as gr
from oracle import mwf_oracle as mo


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'intern_filter_rank_ref.npz'))


def _case(g, i):
    k = int(g['case_pencil'][i])
    a, b = int(g['case_off'][i]), int(g['case_off'][i + 1])
    return (g[f'p{k}_Rxx'], g[f'p{k}_Rnn'], str(g[f'p{k}_kind']), int(g['case_rank'][i]), float(g['case_mu'][i]),
            g['w'][a:b], g['t1'][a:b])


def test_golden_covers_the_issue_grid(golden):
    Ps = {golden[f'p{k}_Rxx'].shape[0] for k in range(int(golden['n_pencils']))}
    assert Ps == {1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16}
    kinds = {str(golden[f'p{k}_kind']) for k in range(int(golden['n_pencils']))}
    assert kinds == {'gap', 'indef', 'corank', 'c64'}
    assert set(np.unique(golden['case_mu'])) == {1.0, 0.3}
    assert {-1, 0, 1, 2} <= set(np.unique(golden['case_rank']).tolist())


def test_closed_form_matches_reference_golden(golden):
    worst = {}
    for i in range(len(golden['case_pencil'])):
        Rxx, Rnn, kind, rank, mu, w_ref, t1_ref = _case(golden, i)
        P = Rxx.shape[0]
        r = gr.kept(rank, P)
        w, t1 = gr.closed_form(Rxx, Rnn, r, mu)
        tol = 1e-9 if Rxx.dtype == np.complex128 else 2e-4
        for nm, got, ref in (('w', w, w_ref), ('t1', t1, t1_ref)):
            e = gr.relerr(got, ref) if np.linalg.norm(ref) > 1e-12 else float(np.abs(got).max())
            assert e < tol, (i, kind, P, rank, mu, nm, e)
            worst[kind] = max(worst.get(kind, 0.0), e)
    print(worst)


@pytest.mark.parametrize('P', [1, 2, 3, 5, 8, 13, 16])
def test_closed_form_matches_oracle_on_gapped_spectra(P):
    rng = np.random.default_rng(100 + P)
    Rxx, Rnn = gr.pencils(rng, 4, P, gr.gapped_spectrum(rng, 4, P))
    for b in range(4):
        for rank in sorted({0, 1, 2, P // 2, P - 1, P, P + 3, -1}):
            for mu in (1.0, 0.3):
                wo, (t1o, _) = mo.intern_filter(Rxx[b], Rnn[b], mu=mu, type='gevd', rank=rank)
                w, t1 = gr.closed_form(Rxx[b], Rnn[b], gr.kept(rank, P), mu)
                assert (gr.relerr(w, wo) if np.linalg.norm(wo) > 0 else float(np.abs(w).max())) < 1e-9, (P, rank, mu)
                assert gr.relerr(t1, t1o) < 1e-9, (P, rank, mu)


def test_slicing_rule():
    from disco_amd.se_utils.internal_formulas import kept_rank
    for P in range(1, 17):
        for rank in range(-P - 3, P + 4):
            D = np.ones(P)
            D[rank:] = 0
            assert kept_rank(rank, P) == gr.kept(rank, P) == int(D.sum()), (P, rank)
        assert kept_rank(np.int64(2), P) == min(2, P)


@pytest.mark.parametrize('rank', [0, 2, -1, np.int64(3)])
def test_mu_zero_with_a_dropped_pair_raises_like_the_reference(rank):
    """The reference's inv(D + 0 I) is singular once a pair is dropped; raised before any device work."""
    from disco_amd.se_utils.internal_formulas import intern_filter, intern_filter_batched
    R = np.eye(4, dtype=np.complex64)
    with pytest.raises(np.linalg.LinAlgError):
        intern_filter(R, R, mu=0, type='gevd', rank=rank)
    with pytest.raises(np.linalg.LinAlgError):
        intern_filter_batched(R[None], R[None], mu=0, rank=rank)
    with pytest.raises(np.linalg.LinAlgError):
        mo.intern_filter(R.astype(np.complex128), R.astype(np.complex128), mu=0, type='gevd', rank=int(rank))


def test_batched_rank_must_be_an_integer():
    from disco_amd.se_utils.internal_formulas import intern_filter_batched
    R = np.eye(3, dtype=np.complex64)[None]
    with pytest.raises(TypeError):
        intern_filter_batched(R, R, rank='Full')
