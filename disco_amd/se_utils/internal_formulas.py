"""`intern_filter` with the reference's signature (disco_theque/se_utils/internal_formulas.py:31-81), on the MI355X.

All three branches run on the GPU: type='gevd' with rank=1 is the one the hot path uses (tango.py:367, 443); 'r1-mwf'
(the function's default type, internal_formulas.py:45-54) and 'mwf' (:74-76) are dead there and offered for
completeness (disco_mwf_filter).  type='gevd' with any other integer rank -- the low-rank GEVD-MWF of Serizel et al. 2014 --
runs the full generalized eigendecomposition (disco_gevd_mwf): the rank is mapped to a kept count by the reference's slicing
rule `D[rank:, :] = 0` (rank >= P: full rank; rank < 0: max(P + rank, 0) kept), and mu = 0 with fewer than P pairs kept raises
numpy.linalg.LinAlgError, as the reference's inv(D + 0 I) does.  An unknown type raises AttributeError and type='gevd' with the
default rank='Full' raises TypeError, exactly like the reference ('full' raises TypeError too, see tests/test_reference_surface_cpu.py)."""
import numpy as np

from .._engines import get_engine

eps = 2.220446049250313e-16      # internal_formulas.py:6
eta = 1e6                        # internal_formulas.py:7


def intern_filter(Rxx, Rnn, mu=1, type='r1-mwf', rank='Full'):
    """Returns (Wint, (t1, sort_index)).  Wint, t1: complex128 (P,) arrays (computed in float64 on the GPU, returned
    through complex64).

    sort_index (type='gevd'; None for the other branches, as in the reference): the reference returns np.argsort(D) of the clamped
    eigenvalues IN THE ORDER scipy.linalg.eig (LAPACK cggev) happened to list them (internal_formulas.py:58-63) -- a permutation that
    refers to an order nobody outside the function ever sees (D and Q are not returned; tango.py:443 binds it and never reads it).
    The GPU solver extracts the dominant pair only and holds no such list; what comes back is the argsort of an ASCENDING list, the
    identity permutation np.arange(P) (int64, like np.argsort): the same type, length and meaning ("position i of the sorted list is
    entry sort_index[i] of the solver's own list"), so code that unpacks and indexes it keeps working; its VALUES cannot be compared
    with the reference's, whose values are LAPACK's ordering accident."""
    if type in ('r1-mwf', 'mwf'):                                             # `rank` is not looked at by these branches
        Rxx = np.ascontiguousarray(Rxx, dtype=np.complex64)
        Rnn = np.ascontiguousarray(Rnn, dtype=np.complex64)
        assert Rxx.shape == Rnn.shape and Rxx.ndim == 2 and Rxx.shape[0] == Rxx.shape[1]
        eng = get_engine(rooms=1, nodes=1, mics=1, length=1024)
        w = eng.mwf_filter(Rxx[None], Rnn[None], type=type, mu=float(mu)).numpy()[0].astype(np.complex128)
        t1 = np.zeros(Rxx.shape[0])
        t1[0] = 1.0                                                           # internal_formulas.py:43 (e1, untouched by these branches)
        return w, (t1, None)
    if type != 'gevd':
        raise AttributeError('Unknown filter reference')                      # internal_formulas.py:79
    if not isinstance(rank, (int, np.integer)):
        raise TypeError("slice indices must be integers (rank='Full' is unusable with type='gevd', as in the reference)")
    Rxx = np.ascontiguousarray(Rxx, dtype=np.complex64)
    Rnn = np.ascontiguousarray(Rnn, dtype=np.complex64)
    assert Rxx.shape == Rnn.shape and Rxx.ndim == 2 and Rxx.shape[0] == Rxx.shape[1]
    w, t1 = _gevd(Rxx[None], Rnn[None], mu, int(rank))
    return w[0].astype(np.complex128), (t1[0].astype(np.complex128), np.arange(Rxx.shape[0], dtype=np.int64))


def kept_rank(rank, P):
    """How many generalized eigenpairs the reference's `D[rank:, :] = 0` keeps of P (Python slicing)."""
    return len(range(P)[:int(rank)])


def _gevd(Rxx, Rnn, mu, rank):
    """(..., P, P) complex64 pencils -> w, t1 (..., P) complex64; rank 1 keeps its own solver (disco_gevd_mwf_r1)."""
    if rank == 1:
        w, t1 = get_engine(rooms=1, nodes=1, mics=1, length=1024).gevd_mwf_r1(Rxx, Rnn, mu=float(mu))
        return w.numpy(), t1.numpy()
    P = Rxx.shape[-1]
    r = kept_rank(rank, P)
    if float(mu) == 0.0 and r < P:
        raise np.linalg.LinAlgError('Singular matrix')                        # inv(D + 0 I) with a dropped pair, as in the reference
    w, t1 = get_engine(rooms=1, nodes=1, mics=1, length=1024).gevd_mwf(Rxx, Rnn, r, mu=float(mu))
    return w.numpy(), t1.numpy()


def intern_filter_batched(Rxx, Rnn, mu=1, rank=1):
    """(..., P, P) pencils -> w, t1 (..., P): the batched form the engine actually runs.  rank: any integer, as in intern_filter."""
    if not isinstance(rank, (int, np.integer)):
        raise TypeError('rank must be an integer')
    Rxx = np.ascontiguousarray(Rxx, dtype=np.complex64)
    Rnn = np.ascontiguousarray(Rnn, dtype=np.complex64)
    return _gevd(Rxx, Rnn, mu, int(rank))
