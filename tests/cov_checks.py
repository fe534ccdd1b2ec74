"""Checks of the masked-covariance kernels pencil by pencil, on every route of disco_cov_masked and disco_step2_cov_fused, through
the staged calls Engine.cov_masked / step2_cov_fused / step2_cov_fused_reuse / gevd_mwf_r1_pending.

Shared by tests/test_gpu_cov_routes.py (real MI355X, `-m gpu`), tests/test_cov_routes_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut down to one room and a few frames) and tests/test_cov_routes_cpu.py (the reference side alone: the route table
against the headers, the exactness of the scenes, the layout helpers).  `make_engine(**cfg)` builds a disco_amd.engine.Engine bound to
the library under test.

Route table (`route` below restates api_cov.hip / api_step2_cov.hip / api_stft_cov.hip; tests/test_cov_routes_cpu.py reads the shape
tables out of the headers and asserts that `exact_cases` launches every name `route` can return):
    disco_cov_masked
        P = M <= 6                              k_cov<M, 0, true, NT>          NT = n_fft / 2 + 64 threads: 320 or 576
        P = M = 7, 8                            k_cov_loc_f64<M>               float64 accumulators, (hi, lo) pairs of partial blocks
        P = M + KR <= 8, KR > 0                 k_cov<M, KR, Zn is Zs, NT>
        9 <= P <= 16, (M, KR) in the split      k_cov_split_lds<M, KR, false>  same z and mask_remote = 1 only
              tables (M = 2, 4, 8)
        9 <= P <= 16, anything else             k_cov_big<Zn is Zs>
        17 <= P <= 32                           k_cov_wide<Zn is Zs>
    disco_step2_cov_fused                       k_step2_cov_fused<M, K, false> every (M, K) with M + K - 1 <= 8
    disco_step2_cov_fused_reuse                 k_step2_cov_fused<M, K, true>  K >= 2
    disco_stft_cov_fused                        k_stft_cov<n_fft, M, true>     M <= 8 at 512 points, M <= 6 at 1024
                                                k_stft + k_cov_loc_f64<M>      M = 7, 8 at 1024 points (the staged pair)
    UNREACHABLE (instantiated, never launched): k_cov<7, 0, ..> and k_cov<8, 0, ..> (both hidden behind k_cov_loc_f64: cov_partials
        walks DISCO_FOR_MKR only when its split test fails, and (7, 0), (8, 0) are in DISCO_FOR_SPLIT_M8), k_cov<M, 0, false, ..> (a step-1 call has no Zn).
    disco_selftest_staged_step2 (through the test-only entry: step 1 on the caller's X, then the staged step 2 of the whole-path calls;
    tests/room_checks.py holds these two, and the re-use route, to the exact tier)
        (M, K) in the room table, "room_cov" = 1  k_room_cov_dma<M, K, 8>        the persistent one-pass room kernel, 6 shapes
        (M, K - 1) in the split tables, K >= 2    k_cov_split_lds<M, KR, true>   the step-1 block skipped, 24 shapes

THE EXACT TIER.  A covariance is a sum of products.  The scenes here hold spectra whose real and imaginary parts are small integers and
masks from {0, 1/4, 1/2, 3/4, 1}: m x, m^2, (1 - m)^2 and every product are multiples of 1/16, so every partial sum -- in any order,
fused or not, in float32 or float64 accumulators, (hi, lo) pairs included -- is exactly representable in float32 as long as 16 x (the
sum over frames of the absolute values of the terms of an entry) stays below 2^24.  `ref_sums` asserts that bound on the float64
reference of every case it builds.  The kernels' unscaled sums must then EQUAL the float64 sums, and what the library hands out is
float32(S * float64(float32(1) / float32(T))):
    T a power of two     Rss, Rnn equal S / T bit for bit
    any other T          per component |got - S/T| <= 1.01 * 2^-23 * |S/T| (one float32 rounding of 1/T, one of the product: 2^-24 each;
                         derived, not measured); a component whose exact sum is 0 comes back exactly 0
    always               R[j, i] is the bitwise conjugate of R[i, j], diagonals have imaginary part exactly 0, z_out of the fused call
                         equals the exact z.
Every comparison is made per (room, node, bin); no bin is excluded.

THE PENDING SOLVES (the solvers' own loaders of the partial blocks: k_solve_small.h, k_solve.h, k_solve_dpp.h, k_solve_wide.h).  The
exact sums make the blocks themselves exact, so a loader that drops, repeats or mis-strides a block solves another pencil.  w and t1
of disco_gevd_mwf_r1_pending are compared per pencil with mwf_oracle.gevd_mwf_r1_hermitian on the exact float64 means.  Bar, per
pencil: 4 x the distance, from that reference, of the same oracle solve fed the means rounded to complex64 (measured on the reference
side, on the inputs of the very case), never lower than 2e-6, the bar check_solver_sizes holds these solvers to.  The scenes are built
so that more than nine pencils in ten are held to that floor (asserted).

Which solver's loader reads which family's blocks is the table PENDING (every one of the four is reached).  This bar is recomputed on
the inputs of every run, not committed as a table.

THE RE-USE ROUTE (disco_step2_cov_fused_reuse) hands out no matrices and, after disco_stft_cov_fused, works on transformed spectra that
cannot be exact: `check_reuse` holds its z_out bit-identical to the non-reuse call's and compares its pending solve per pencil on all 28
shapes, with the float32 restatement of the sums as the reference-side perturbation.  (tests/room_checks.py `check_reuse_exact` holds the
same kernel to the exact tier: step 1 established by disco_cov_masked on an exact scene, the matrices read by the test-only
disco_selftest_pending_matrices.)  THE FLOAT TIERS (the staged families at 626
frames in one chunk; disco_stft_cov_fused against the complex128 transform) are described above `check_float` and `check_stft_cov`.
"""
import re

import numpy as np

from oracle import mwf_oracle as mo

HOP = {512: 256, 1024: 512}
MASK_VALUES = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
MEAN_TOL = 1.01 * 2.0 ** -23
SOLVE_FLOOR = 2e-6
BAR_FACTOR = 4.0

# ---- the shape tables of the dispatch, restated (tests/test_cov_routes_cpu.py compares them with the headers) ---------------------------

MKR = tuple((m, kr) for m in range(1, 9) for kr in range(0, 9 - m))                    # DISCO_FOR_MKR (dispatch.h)
SPLIT = ((7, 0), (8, 0)) + tuple((8, kr) for kr in range(1, 9)) + tuple((4, kr) for kr in range(5, 13)) \
    + tuple((2, kr) for kr in range(7, 15))                                            # DISCO_FOR_SPLIT_M8 / M4 / M2 (dispatch.h)
CB_PMAX, CW_PMAX = 16, 32

UNREACHABLE = tuple(f'k_cov<{m},0,{s},{nt}>' for m in (7, 8) for s in ('true', 'false') for nt in (320, 576)) \
    + tuple(f'k_cov<{m},0,false,{nt}>' for m in range(1, 7) for nt in (320, 576))
ROOM = ((8, 8), (8, 6), (8, 4), (8, 2), (4, 8), (4, 6))                                # DISCO_FOR_ROOM (dispatch.h): (M, K); SUB = 8 (api_room_s8.hip)


def selftest_reachable():
    """The kernels only disco_selftest_staged_step2 reaches from a staged call (tests/room_checks.py runs them)."""
    return {f'k_room_cov_dma<{M},{K},8>' for M, K in ROOM} | {f'k_cov_split_lds<{M},{KR},true>' for M, KR in SPLIT if KR > 0}


def _b(x):
    return 'true' if x else 'false'


def route(M, K, n_fft, step2, same_z=True, mask_remote=True, call='cov_masked'):
    """The kernel(s) a call launches, as a tuple of names; a refusal as ('refused: ...',).  call: 'cov_masked' (step2: P = M + K - 1,
    else P = M), 'step2_fused', 'step2_reuse', 'stft_cov' ('k_stft' there stands for the plain transform, k_stft or k_stft_pairs)."""
    assert n_fft in (512, 1024)
    nt = n_fft // 2 + 64
    if call == 'stft_cov':
        if M > 8:
            return ('refused: more than 8 mics',)
        if n_fft == 1024 and M > 6:
            return ('k_stft', f'k_cov_loc_f64<{M}>')
        return (f'k_stft_cov<{n_fft},{M},true>',)
    if call in ('step2_fused', 'step2_reuse'):
        if M + K - 1 > 8:
            return ('refused: M + K - 1 > 8',)
        if call == 'step2_reuse' and K < 2:
            return ('refused: one node',)
        return (f'k_step2_cov_fused<{M},{K},{_b(call == "step2_reuse")}>',)
    assert call == 'cov_masked'
    KR = K - 1 if step2 else 0
    P = M + KR
    if M > 8:
        return ('refused: M > 8',)
    if P > CW_PMAX:
        return ('refused: P > 32',)
    same = same_z or KR == 0
    if P > CB_PMAX:
        return (f'k_cov_wide<{_b(same)}>',)
    if (KR == 0 or (P > 8 and same and mask_remote)) and (M, KR) in SPLIT:
        return (f'k_cov_loc_f64<{M}>',) if KR == 0 else (f'k_cov_split_lds<{M},{KR},false>',)
    if (M, KR) in MKR:
        return (f'k_cov<{M},{KR},{_b(same)},{nt}>',)
    return (f'k_cov_big<{_b(same)}>',)


def reachable(selftest=True):
    """Every kernel name `route` can return for a staged covariance call (the exact tier's and the re-use route's) and, with `selftest`,
    the ones the test-only entry adds."""
    names = selftest_reachable() if selftest else set()
    for n_fft in (512, 1024):
        for M in range(1, 9):
            for K in range(1, 34):
                for same in (True, False):
                    for mr in (True, False):
                        for step2 in (False, True):
                            names.update(route(M, K, n_fft, step2, same, mr))
                for call in ('step2_fused', 'step2_reuse'):
                    names.update(route(M, K, n_fft, True, call=call))
    return {n for n in names if not n.startswith('refused')}


def kernel_key(traced_name):
    """A kernel name of a trace ('void disco::k_cov<2, 3, true, 320>(disco::CovArgs)') in the form `route` writes."""
    s = re.sub(r'\(.*$', '', traced_name.strip().replace('void ', '')).replace('disco::', '').replace(' ', '')
    return re.sub(r'\((bool|int)\)', '', s)


# ---- the list of cases --------------------------------------------------------------------------------------------------------------

def exact_cases(cut=False):
    """dicts of keyword arguments of `check_staged` / `check_fused` ('call': 'cov_masked' | 'step2_fused').  cut: the emulator's list --
    every family, every M of k_cov and k_step2_cov_fused, far fewer crossings."""
    cases = []

    def add(M, K, n_fft=512, step2=True, same_z=True, mask_remote=True, call='cov_masked'):
        c = dict(M=M, K=K, n_fft=n_fft, step2=step2, same_z=same_z, mask_remote=mask_remote, call=call)
        if c not in cases:
            cases.append(c)
    if cut:
        for M in range(1, 9):
            add(M, 1, step2=False)
        add(3, 1, 1024, step2=False)
        add(8, 1, 1024, step2=False)
        for M in range(1, 8):                                            # every M of k_cov with remote rows; both SAMEZ forms
            add(M, 9 - M if M % 2 else 2, same_z=bool(M % 2), mask_remote=M % 3 != 0)
        add(2, 3, 1024, same_z=False)
        for M, K in ((8, 2), (4, 6), (2, 15)):                           # k_cov_split_lds: first / last shape of the three tables
            add(M, K)
        add(4, 13)
        add(8, 2, same_z=False)                                          # k_cov_big<false>
        add(4, 6, mask_remote=False)                                     # k_cov_big<true>
        add(3, 8)
        add(1, 16, same_z=False, mask_remote=False)
        add(7, 3)
        add(1, 17)                                                       # k_cov_wide
        add(8, 25)
        add(5, 14, same_z=False)
        add(3, 20, mask_remote=False)
        for M in range(1, 9):                                            # every M of k_step2_cov_fused
            add(M, min(9 - M, 3) if M < 8 else 1, call='step2_fused')
        add(1, 8, call='step2_fused')
        add(2, 2, 1024, call='step2_fused')
        return cases
    for n_fft in (512, 1024):                                            # step 1: k_cov<M, 0>, k_cov_loc_f64<7>, <8>
        for M in range(1, 9):
            add(M, 1, n_fft, step2=False)
    for M, KR in MKR:                                                    # step 2, P <= 8: all 28 shapes x same / distinct z x mask_remote
        if KR > 0:
            for same in (True, False):
                for mr in (True, False):
                    add(M, KR + 1, 512, same_z=same, mask_remote=mr)
    for i, (M, KR) in enumerate(MKR):                                    # ... at 1024 points: both SAMEZ forms of every shape (they are
        if KR > 0:                                                       # instantiations of their own), mask_remote alternating
            add(M, KR + 1, 1024, same_z=True, mask_remote=bool(i % 2))
            add(M, KR + 1, 1024, same_z=False, mask_remote=not i % 2)
    for M, KR in SPLIT:                                                  # P = 9 .. 16: the 24 split shapes, and the same shapes through
        if KR > 0:                                                       # k_cov_big<false> (distinct Zn) and <true> (mask_remote = 0)
            add(M, KR + 1)
            add(M, KR + 1, same_z=False)
            add(M, KR + 1, mask_remote=False)
    add(8, 2, 1024)
    add(4, 9, 1024)
    add(2, 15, 1024)
    for M, K in ((1, 9), (3, 8), (5, 7), (7, 6), (3, 11), (5, 10), (7, 2 + 7), (1, 16), (7, 10), (6, 4), (7, 3), (6, 11), (3, 12), (5, 9)):
        add(M, K)                                                        # outside the split tables: P = 9 .. 16 through k_cov_big<true>
        add(M, K, same_z=False, mask_remote=bool(M % 4 != 1))            # ... and <false>
    add(1, 16, same_z=False, mask_remote=False)
    add(7, 3, 1024)
    add(5, 8, 1024, same_z=False)
    for P in range(17, 33):                                              # P = 17 .. 32: every P through k_cov_wide<true>
        M = 1 + (P * 5) % 8
        add(M, P - M + 1)
    add(8, 25, 1024)
    for M, K, same, mr in ((1, 17, False, True), (8, 12, False, False), (4, 20, True, False), (5, 28, False, True), (2, 31, True, False)):
        add(M, K, same_z=same, mask_remote=mr)
    for M, KR in MKR:                                                    # disco_step2_cov_fused: every instantiation
        add(M, KR + 1, call='step2_fused')
    for M, K in ((1, 2), (2, 3), (4, 4), (1, 8), (7, 2), (8, 1)):
        add(M, K, 1024, call='step2_fused')
    return cases


CASE_FAMILIES = ('k_cov_step1', 'k_cov', 'k_cov_loc_f64', 'k_cov_split_lds', 'k_cov_big', 'k_cov_wide', 'k_step2_cov_fused')


def family_of(case):
    name = route(case['M'], case['K'], case['n_fft'], case['step2'], case['same_z'], case['mask_remote'], call=case.get('call', 'cov_masked'))[0]
    fam = name.split('<')[0]
    return 'k_cov_step1' if fam == 'k_cov' and not case['step2'] else fam


def reuse_shapes():
    """Every (M, K >= 2) with M + K - 1 <= 8: the shapes of disco_step2_cov_fused_reuse."""
    return [(M, KR + 1) for M, KR in MKR if KR > 0]


def launched_by(cases):
    names = set()
    for c in cases:
        call = c.get('call', 'cov_masked')
        names.update(route(c['M'], c['K'], c['n_fft'], c['step2'], c['same_z'], c['mask_remote'], call=call))
    return names


# ---- scenes whose sums are exact -----------------------------------------------------------------------------------------------------

def _cint(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32) + 1j * rng.integers(lo, hi + 1, shape).astype(np.float32)


def scene(seed, R, K, M, T, F, step2=True, solvable=False):
    """-> X (R, K, T, F, M) c64, Zs, Zn (R, K, T, F) c64 (None unless step2), mask (R, K, T, F) f32.
    Per bin one integer source times an integer steering vector plus integer noise on every row (full-rank pencils, not all alike); z
    rows drawn independently per (room, node), so a row read at a wrong node or room changes the sums; masks from MASK_VALUES with whole
    bins of exact 0 and exact 1.  solvable (the pending solves): the source is on or off per (frame, bin) and the masks, from {1/4, 1/2,
    3/4} only, follow it: both matrices of every pencil are definite and the top eigenvalue stands clear of the rest."""
    rng = np.random.default_rng(seed)
    steer = 2 * _cint(rng, 0, 1, (R, K, 1, F, M)) - (1 + 1j)               # parts from {-1, 1}: no channel without the source
    src = _cint(rng, -1, 1, (R, 1, T, F, 1))
    act = rng.integers(0, 2, (R, 1, T, F, 1))
    if solvable:
        src = (2 * _cint(rng, 0, 1, (R, 1, T, F, 1)) - (1 + 1j)) * act
    X = (steer * src + _cint(rng, -1, 1, (R, K, T, F, M))).astype(np.complex64)
    Zs = Zn = None
    if step2:
        Zs = _cint(rng, -2, 2, (R, K, T, F)).astype(np.complex64)
        Zn = _cint(rng, -2, 2, (R, K, T, F)).astype(np.complex64)
    if solvable:                                                          # 3/4 or 1/2 where the source is on, 1/4 or 1/2 where it is off
        a = np.broadcast_to(act[..., 0], (R, K, T, F))
        mask = MASK_VALUES[np.where(a == 1, rng.integers(2, 4, (R, K, T, F)), rng.integers(1, 3, (R, K, T, F)))]
    else:
        mask = MASK_VALUES[rng.integers(0, 5, (R, K, T, F))]
        f = np.arange(F)[None, None, :]
        sel = (f + np.arange(R)[:, None, None] + 3 * np.arange(K)[None, :, None]) % 7
        mask = np.where((sel == 3)[:, :, None, :], np.float32(0), mask)
        mask = np.where((sel == 5)[:, :, None, :], np.float32(1), mask)
    return X, Zs, Zn, np.ascontiguousarray(mask.astype(np.float32))


def sparse_filters(seed, R, K, F, M):
    """Integer w_loc (R, K, F, M) with at most two entries from {1, -1, i, -i} per filter: z = w^H x stays a small integer."""
    rng = np.random.default_rng(seed)
    w = np.zeros((R, K, F, M), np.complex64)
    units = np.array([1, -1, 1j, -1j], np.complex64)
    idx = np.indices((R, K, F))
    for _ in range(2):
        m = rng.integers(0, M, (R, K, F))
        w[idx[0], idx[1], idx[2], m] = units[rng.integers(0, 4, (R, K, F))]
    return w


def z_to_blocks(Z, zblk):
    """Z (R, K, T, F) in the plain layout -> the rank-major layout disco_set_z_blocks names: [K / zblk][R][zblk][T][F]."""
    R, K = Z.shape[:2]
    assert K % zblk == 0
    return np.ascontiguousarray(Z.reshape(R, K // zblk, zblk, *Z.shape[2:]).swapaxes(0, 1))


def z_plane(r, j, R, zblk):
    """Index of the (T, F) plane of room r, global node j in the layout above (common.h z_plane)."""
    return (j // zblk * R + r) * zblk + j % zblk


def rows_of(X, Z, r, k, kl):
    """(T, F, P): [X_k ; z_j, j < k ; z_j, j > k] (concatenate_signals, tango.py:142-155) of global node k, held at local index kl."""
    rows = [X[r, kl].astype(np.complex128)]
    if Z is not None:
        K = Z.shape[1]
        others = [j for j in range(K) if j != k]
        if others:
            rows.append(np.stack([Z[r, j].astype(np.complex128) for j in others], axis=-1))
    return np.concatenate(rows, axis=-1)


def ref_sums(X, mask, Zs=None, Zn=None, mask_remote=True, nodes=None, frames=None):
    """float64 restatement of tango.py:357-364 / 433-440 WITHOUT the division by T: -> Sss, Snn (R, Kl, F, P, P) complex128, the sums
    over the frames t < frames[r] (all T by default).  X / mask hold the nodes `nodes` (global indices; all K by default), Zs / Zn all
    K.  Asserts the representability bound of the exact tier: 16 x sum_t (|re| + |im|)^2 of every weighted row below 2^24 (by
    Cauchy-Schwarz that bounds the sum of the absolute values of the terms of every entry)."""
    R, Kl, T, F, M = X.shape
    nodes = list(range(Kl)) if nodes is None else list(nodes)
    assert len(nodes) == Kl
    P = M + ((Zs.shape[1] - 1) if Zs is not None else 0)
    Sss = np.zeros((R, Kl, F, P, P), np.complex128)
    Snn = np.zeros_like(Sss)
    worst = 0.0
    for r in range(R):
        Tr = T if frames is None else int(frames[r])
        for kl, k in enumerate(nodes):
            m = mask[r, kl, :Tr].astype(np.float64)[..., None]
            vs = rows_of(X, Zs, r, k, kl)[:Tr]
            vn = vs if Zn is Zs else rows_of(X, Zn, r, k, kl)[:Tr]
            ws = np.repeat(m, P, axis=-1)
            wn = 1.0 - ws
            if not mask_remote:
                ws[..., M:] = 1.0
                wn[..., M:] = 1.0
            vs = np.ascontiguousarray((ws * vs).transpose(1, 2, 0))                    # (F, P, Tr)
            vn = np.ascontiguousarray((wn * vn).transpose(1, 2, 0))
            Sss[r, kl] = vs @ vs.conj().transpose(0, 2, 1)
            Snn[r, kl] = vn @ vn.conj().transpose(0, 2, 1)
            for v in (vs, vn):
                worst = max(worst, float((16.0 * ((np.abs(v.real) + np.abs(v.imag)) ** 2).sum(-1)).max()))
    assert worst < 2.0 ** 24, f'test bug: the scene breaks the representability bound ({worst:.3g} >= 2^24)'
    # multiples of 1/16 all along: the float64 sums are the exact sums
    assert np.array_equal(Sss * 16, np.round(Sss * 16)) and np.array_equal(Snn * 16, np.round(Snn * 16))
    return Sss, Snn


def f32_sequential_sums(X, mask, r, k, f):
    """The step-1 sums of one (room, node, bin) accumulated frame by frame in float32 (NumPy, no kernel): what the exact tier claims
    equals the float64 sums bit for bit.  -> Sss, Snn (M, M) complex64."""
    T, M = X.shape[2], X.shape[4]
    ss = np.zeros((M, M), np.complex64)
    nn = np.zeros((M, M), np.complex64)
    for t in range(T):
        m = np.float32(mask[r, k, t, f])
        vs = (m * X[r, k, t, f]).astype(np.complex64)
        vn = ((np.float32(1) - m) * X[r, k, t, f]).astype(np.complex64)
        ss = (ss + np.outer(vs, vs.conj()).astype(np.complex64)).astype(np.complex64)
        nn = (nn + np.outer(vn, vn.conj()).astype(np.complex64)).astype(np.complex64)
    return ss, nn


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _first_bad(bad, n=4):
    """bad: (R, K, F) bool -> a short description of the failing pencils."""
    idx = np.argwhere(bad)
    return f'{len(idx)} of {bad.size} pencils, first (room, node, bin): {[tuple(int(v) for v in i) for i in idx[:n]]}'


def compare_exact(got, S, frames, what):
    """got (R, Kl, F, P, P) complex64 from the library, S the exact sums, frames (R,) the divisor of every room.  Per pencil."""
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == S.shape, (got.dtype, got.shape, S.shape)
    R, Kl, F, P, _ = S.shape
    for r in range(R):
        Tr = int(frames[r])
        ref = S[r] / Tr
        g = got[r]
        if Tr & (Tr - 1) == 0:                                           # a power of two: exact
            want = ref.astype(np.complex64)
            assert np.array_equal(want.astype(np.complex128), ref)
            bad = (g.real != want.real) | (g.imag != want.imag)
        else:
            bad = np.zeros(ref.shape, bool)
            for gc, rc in ((g.real.astype(np.float64), ref.real), (g.imag.astype(np.float64), ref.imag)):
                bad |= ~(np.abs(gc - rc) <= MEAN_TOL * np.abs(rc))        # an exact 0 must come back 0; NaN fails
        bad_pencil = bad.any(axis=(-1, -2))
        if bad_pencil.any():
            k, f = (int(v) for v in np.argwhere(bad_pencil)[0])
            ij = [tuple(int(v) for v in e) for e in np.argwhere(bad[k, f])[:6]]
            raise AssertionError(f'{what}: room {r} (T_r = {Tr}): {_first_bad(bad_pencil[None])}; at node {k} bin {f} entries {ij}: got '
                                 f'{[complex(g[k, f][e]) for e in ij]}, exact mean {[complex(ref[k, f][e]) for e in ij]} '
                                 f'(difference x T_r = {[complex(g[k, f][e]) * Tr - complex(S[r, k, f][e]) for e in ij]})')
    # Hermitian to the bit: R[j, i] = conj(R[i, j]) (float equality: bit equality but for the sign of a zero); real diagonal
    gt = np.swapaxes(got, -1, -2)
    bad = ~((got.real == gt.real) & (got.imag == -gt.imag))
    bad |= (got.imag != 0) & np.eye(P, dtype=bool)
    assert not bad.any(), f'{what}: not Hermitian to the bit: {_first_bad(bad.any(axis=(-1, -2)))}'


def _engine(make_engine, R, K, M, T, n_fft, pad=None):
    hop = HOP[n_fft]
    L = max(1, (T - 1) * hop)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft, pad_mode=pad or ('constant' if L <= n_fft // 2 else 'reflect'))
    assert eng.T == T and eng.F == n_fft // 2 + 1, (eng.T, T)
    return eng


def _seed(*key):
    return int(np.uint32(hash(tuple(int(k) for k in key)) & 0x7fffffff))


def check_staged(make_engine, M, K, n_fft=512, step2=True, same_z=True, mask_remote=True, T=64, R=1, chunks=0, shard=None, zblk=None,
                 lengths_frames=None, **_):
    """disco_cov_masked on an exact scene, every pencil against the exact sums.  shard: (k0, Kl); zblk: rank-major z blocks;
    lengths_frames: per-room T_r (set_lengths, X zeroed beyond them as the header asks of a caller)."""
    F = n_fft // 2 + 1
    X, Zs, Zn, mask = scene(_seed(M, K, n_fft, step2, T, R), R, K, M, T, F, step2)
    if same_z:
        Zn = Zs
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if lengths_frames is not None else None)
    try:
        if chunks:
            eng.set_tuning(cov_chunks=chunks)
        frames = np.full(R, T)
        if lengths_frames is not None:
            frames = np.asarray(lengths_frames)
            eng.set_lengths([(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in frames])
            assert np.array_equal(eng.frames, frames)
            for r in range(R):
                X[r, :, frames[r]:] = 0
                if step2:                                 # the z of a room are its own spectra filtered: zeros beyond its frames too
                    Zs[r, :, frames[r]:] = 0
                    Zn[r, :, frames[r]:] = 0
        nodes = list(range(K))
        Xl, ml = X, mask
        if shard is not None:
            k0, Kl = shard
            eng.set_node_shard(k0, Kl)
            nodes = list(range(k0, k0 + Kl))
            Xl, ml = np.ascontiguousarray(X[:, nodes]), np.ascontiguousarray(mask[:, nodes])
        zs_in, zn_in = Zs, Zn
        if zblk is not None:
            eng.set_z_blocks(zblk)
            zs_in = z_to_blocks(Zs, zblk)
            zn_in = zs_in if same_z else z_to_blocks(Zn, zblk)
        Rss, Rnn = eng.cov_masked(Xl, ml, zs_in, zn_in, mask_remote=mask_remote)
        Rss, Rnn = Rss.numpy(), Rnn.numpy()
        Sss, Snn = ref_sums(Xl, ml, Zs, Zn, mask_remote, nodes=nodes, frames=frames)
        what = f'{route(M, K, n_fft, step2, same_z, mask_remote)[0]} (M={M} K={K} n_fft={n_fft} T={T} R={R} chunks={chunks} shard={shard} zblk={zblk})'
        compare_exact(Rss, Sss, frames, what + ' Rss')
        compare_exact(Rnn, Snn, frames, what + ' Rnn')
    finally:
        eng.close()
    return Rss.shape


def check_fused(make_engine, M, K, n_fft=512, T=64, R=1, chunks=0, lengths_frames=None, **_):
    """disco_step2_cov_fused on an exact scene with integer w_loc: z_out and every pencil against the exact values."""
    F = n_fft // 2 + 1
    X, _zs, _zn, mask = scene(_seed(M, K, n_fft, 7, T, R), R, K, M, T, F, False)
    w_loc = sparse_filters(_seed(M, K, 11), R, K, F, M)
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if lengths_frames is not None else None)
    try:
        if chunks:
            eng.set_tuning(step2_chunks=chunks)
        frames = np.full(R, T)
        if lengths_frames is not None:
            frames = np.asarray(lengths_frames)
            eng.set_lengths([(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in frames])
            for r in range(R):
                X[r, :, frames[r]:] = 0
        z_ref = np.einsum('rkfm,rktfm->rktf', w_loc.conj().astype(np.complex128), X.astype(np.complex128))
        Rss, Rnn, z = eng.step2_cov_fused(X, mask, w_loc, want_z=True)
        Rss, Rnn, z = Rss.numpy(), Rnn.numpy(), z.numpy()
        what = f'k_step2_cov_fused<{M},{K},false> (n_fft={n_fft} T={T} R={R} chunks={chunks} frames={lengths_frames})'
        bad = (z.astype(np.complex128) != z_ref).any(axis=2)
        assert not bad.any(), f'{what}: z_out differs from the exact z: {_first_bad(bad)}'
        zc = z_ref.astype(np.complex64) if K > 1 else None
        Sss, Snn = ref_sums(X, mask, zc, zc, True, frames=frames)
        compare_exact(Rss, Sss, frames, what + ' Rss')
        compare_exact(Rnn, Snn, frames, what + ' Rnn')
    finally:
        eng.close()
    return Rss.shape


def check_case(make_engine, case, **over):
    c = dict(case, **over)
    return (check_fused if c.get('call') == 'step2_fused' else check_staged)(make_engine, **c)


def check_exact_cases(make_engine, cases, **over):
    names = set()
    for c in cases:
        check_case(make_engine, c, **over)
        names.update(route(c['M'], c['K'], c['n_fft'], c['step2'], c['same_z'], c['mask_remote'], call=c.get('call', 'cov_masked')))
    return sorted(names)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------

FAMILIES = {                                   # one shape per kernel family: (M, K, step2)
    'k_cov': (2, 3, True),
    'k_cov_loc_f64': (7, 1, False),
    'k_cov_big': (3, 8, True),
    'k_cov_split_lds': (2, 8, True),
    'k_cov_wide': (2, 17, True),
}
FUSED_SHAPE = (2, 3)
# (T, chunk count pinned; 0 = the heuristic): chunk lengths of exactly 64 (T = 64 in one, 128 in two), 65 (65 in one, 130 in two), 129
# (129 in one, 258 in two); T not divisible by the count; T < the count; T = 626 in one chunk
GEOMETRY = ((1, 0), (1, 8), (2, 0), (2, 3), (3, 2), (3, 7), (63, 0), (63, 7), (63, 1), (64, 1), (64, 3), (65, 1), (65, 2), (129, 1),
            (129, 8), (128, 2), (130, 2), (258, 2), (626, 1), (626, 3), (2, 700))
GEOMETRY_CUT = ((1, 0), (2, 3), (3, 2), (5, 7), (66, 1))                # the emulator's: one chunk longer than 64 frames


def chunk_lengths(T, chunks):
    c = max(1, min(chunks, T))
    return [T * (i + 1) // c - T * i // c for i in range(c)]


def check_geometry(make_engine, geometry=GEOMETRY, families=None, long_families=None):
    """Every family at every (T, chunk count) of `geometry`.  long_families (the emulator's cut): the only families that run the
    entries of more than 64 frames."""
    done = []
    for name, (M, K, step2) in list(FAMILIES.items()) + [('k_step2_cov_fused', FUSED_SHAPE + (True,))]:
        if families is not None and name not in families:
            continue
        for T, chunks in geometry:
            if long_families is not None and T > 64 and name not in long_families:
                continue
            if name == 'k_step2_cov_fused':
                check_fused(make_engine, M, K, 512, T=T, chunks=chunks)
            else:
                check_staged(make_engine, M, K, 512, step2, T=T, chunks=chunks)
            done.append((name, T, chunks))
    return done


def check_default_single_chunk(make_engine, R=1024, K=2, M=1, T=3):
    """R x K >= 2048 units and few frames: the default heuristic itself picks one chunk (cov_chunks: ceil(2048 / (R K)) = 1)."""
    assert R * K >= 2048
    check_staged(make_engine, M, K, 512, True, T=T, R=R)
    check_fused(make_engine, M, K, 512, T=T, R=R)


# ---- node shards, z layout, per-room lengths ------------------------------------------------------------------------------------------

def check_shards(make_engine, T=64, every_k0=True, wide=True):
    """set_node_shard at every k0 of a K = 4 and a K = 6 room (one node and a pair), rank-major z blocks, through k_cov, k_cov_big and
    k_cov_split_lds; a wide network through k_cov_wide at its first, a middle and its last k0."""
    done = []
    plan = [(2, 4, None), (2, 6, None), (5, 6, None), (8, 4, None), (4, 6, None)]     # k_cov x 2, k_cov_big, k_cov_split_lds x 2
    for M, K, _n in plan:
        k0s = range(K) if every_k0 else (0, K - 1)
        for k0 in k0s:
            check_staged(make_engine, M, K, 512, True, T=T, shard=(k0, 1))
            done.append((M, K, k0, 1, None))
        for k0 in (range(0, K, 2) if every_k0 else (K - 2,)):
            check_staged(make_engine, M, K, 512, True, T=T, R=2, shard=(k0, 2), zblk=2, same_z=(k0 % 4 == 0))
            done.append((M, K, k0, 2, 2))
        check_staged(make_engine, M, K, 512, True, T=T, R=2, zblk=K // 2)               # all nodes here, rank-major z
        done.append((M, K, 0, K, K // 2))
    if wide:
        M, K = 2, 18
        for k0 in (0, 9, 17):
            check_staged(make_engine, M, K, 512, True, T=T, R=2, shard=(k0, 1), zblk=3 if k0 else None)
            done.append((M, K, k0, 1, 3 if k0 else None))
    return done


def check_lengths(make_engine, T=64, chunks=4):
    """Per-room lengths: every room's matrices are the mean over its OWN frames.  With T = 64 in 4 chunks of 16: a room that ends inside
    a chunk (T_r = 37), one that ends before a whole chunk (T_r = 16: chunks 1 .. 3 empty), a full room, a one-frame room."""
    frames = [37, 16, T, 1] if T >= 64 else [T - 1, 1, T, 2]
    done = []
    for name, (M, K, step2) in FAMILIES.items():
        check_staged(make_engine, M, K, 512, step2, T=T, R=4, chunks=chunks, lengths_frames=frames)
        done.append(name)
    check_fused(make_engine, *FUSED_SHAPE, 512, T=T, R=4, chunks=chunks, lengths_frames=frames)
    check_fused(make_engine, 4, 4, 512, T=T, R=4, chunks=chunks, lengths_frames=frames[::-1])
    return done + ['k_step2_cov_fused']


# ---- a non-finite input stays where it is ---------------------------------------------------------------------------------------------

def check_nonfinite(make_engine, T=16, families=None):
    """One NaN in one (room, node, frame, bin) of X (and of that node's z row): every pencil of another bin, another room, and of a node
    that does not receive the NaN through a z row is bit-identical to the clean run."""
    R = 2
    r0, k0, f0 = 1, 1, 37
    for name, (M, K, step2) in FAMILIES.items():
        if families is not None and name not in families:
            continue
        F = 257
        X, Zs, _zn, mask = scene(_seed(M, K, 5), R, K, M, T, F, step2)
        eng = _engine(make_engine, R, K, M, T, 512)
        try:
            eng.set_tuning(cov_chunks=3)
            clean = [a.numpy() for a in eng.cov_masked(X, mask, Zs, Zs)]
            kk = min(k0, K - 1)
            Xn = X.copy()
            Xn[r0, kk, T // 2, f0, M - 1] = np.nan
            hit_x = [a.numpy() for a in eng.cov_masked(Xn, mask, Zs, Zs)]
            same = np.ones((R, K, F), bool)
            same[r0, kk, f0] = False                                     # the NaN's own pencil; z rows are clean: no other node sees it
            for c, h in zip(clean, hit_x):
                eq = (_bits(c).reshape(c.shape + (2,)) == _bits(h).reshape(h.shape + (2,))).all(axis=(-1, -2, -3))
                assert eq[same].all(), f'{name}: a NaN in X moved {_first_bad(~eq & same)}'
                assert np.isnan(h[r0, kk, f0]).any(), f'{name}: the NaN did not reach its own pencil'
            if step2:
                Zh = Zs.copy()
                Zh[r0, kk, T // 2, f0] = np.nan                          # every OTHER node of that room receives it, at that bin only
                hit_z = [a.numpy() for a in eng.cov_masked(X, mask, Zh, Zh)]
                same = np.ones((R, K, F), bool)
                same[r0, :, f0] = False
                same[r0, kk, f0] = True                                  # a node does not read its own z row
                for c, h in zip(clean, hit_z):
                    eq = (_bits(c).reshape(c.shape + (2,)) == _bits(h).reshape(h.shape + (2,))).all(axis=(-1, -2, -3))
                    assert eq[same].all(), f'{name}: a NaN in a z row moved {_first_bad(~eq & same)}'
        finally:
            eng.close()
    if families is None or 'k_step2_cov_fused' in families:
        M, K = FUSED_SHAPE
        X, _a, _b2, mask = scene(_seed(M, K, 6), R, K, M, T, 257, False)
        w = sparse_filters(3, R, K, 257, M)
        eng = _engine(make_engine, R, K, M, T, 512)
        try:
            eng.set_tuning(step2_chunks=3)
            clean = [a.numpy() for a in eng.step2_cov_fused(X, mask, w)]
            Xn = X.copy()
            Xn[r0, 1, T // 2, f0, :] = np.nan                            # whatever w_loc picks: z of node 1 is NaN there
            hit = [a.numpy() for a in eng.step2_cov_fused(Xn, mask, w)]
            same = np.ones((R, K, 257), bool)
            same[r0, :, f0] = False                                      # every node of the room receives it through z
            for c, h in zip(clean[:2], hit[:2]):
                eq = (_bits(c).reshape(c.shape + (2,)) == _bits(h).reshape(h.shape + (2,))).all(axis=(-1, -2, -3))
                assert eq[same].all(), f'k_step2_cov_fused: a NaN in X moved {_first_bad(~eq & same)}'
            zc, zh = clean[2], hit[2]
            neq = (_bits(zc) != _bits(zh)).reshape(zc.shape + (2,)).any(axis=-1)
            assert neq[r0, 1, T // 2, f0]
            neq[r0, 1, T // 2, f0] = False
            assert not neq.any(), 'k_step2_cov_fused: z_out changed away from the NaN'
        finally:
            eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def check_refusals(make_engine):
    """Each refusal returns its documented error (-1 DISCO_E_ARG, -2 DISCO_E_UNSUPPORTED) and leaves the context usable."""
    def raw_cov(eng, X, mask, Zs, Zn, P, Rss=True, Rnn=True):
        px, kx = eng.to_device(X, np.complex64)
        pm, km = eng.to_device(mask, np.float32)
        pzs, k1 = eng.to_device(Zs, np.complex64)
        pzn, k2 = eng.to_device(Zn, np.complex64)
        out = eng.empty((eng.R * eng.Kl * eng.F * P * P,), np.complex64)
        rc = eng.lib.disco_cov_masked(eng.ctx, px, pm, pzs, pzn, 1, P, out.ptr if Rss else None, out.ptr if Rnn else None, eng.stream)
        return rc, eng.lib.disco_last_error(eng.ctx).decode()

    def usable(eng, X, mask, Zs):
        Rss, Rnn = eng.cov_masked(X, mask, Zs, Zs)
        Sss, _ = ref_sums(X, mask, Zs, Zs)
        compare_exact(Rss.numpy(), Sss, np.full(X.shape[0], X.shape[2]), 'after a refusal')

    T, F = 4, 257
    X, Zs, Zn, mask = scene(1, 1, 3, 2, T, F, True)
    eng = _engine(make_engine, 1, 3, 2, T, 512)
    try:
        rc, msg = raw_cov(eng, X, mask, Zs, Zs, 3)                       # P neither M (2) nor M + K - 1 (4)
        assert rc == -1 and 'P must be M or M + K - 1' in msg, (rc, msg)
        rc, msg = raw_cov(eng, X, mask, Zs, None, 4)                     # Zs without Zn
        assert rc == -1 and 'Zs/Zn required' in msg, (rc, msg)
        rc, msg = raw_cov(eng, X, mask, Zs, Zs, 4, Rnn=False)            # only one of Rss / Rnn
        assert rc == -1 and 'both' in msg, (rc, msg)
        rc, msg = raw_cov(eng, X, mask, Zs, Zs, 4, Rss=False)
        assert rc == -1 and 'both' in msg, (rc, msg)
        usable(eng, X, mask, Zs)
        eng.set_node_shard(1, 1)                                         # the fused step 2 under a node shard
        px, kx = eng.to_device(X, np.complex64)
        pm, km = eng.to_device(mask, np.float32)
        pw, kw = eng.to_device(sparse_filters(1, 1, 3, F, 2), np.complex64)
        out = eng.empty((3 * F * 16,), np.complex64)
        rc = eng.lib.disco_step2_cov_fused(eng.ctx, px, pm, pw, None, out.ptr, out.ptr, eng.stream)
        assert rc == -2 and 'node shard' in eng.lib.disco_last_error(eng.ctx).decode(), rc
        eng.set_node_shard(0, 3)
        usable(eng, X, mask, Zs)
    finally:
        eng.close()
    for M, K, P, want in ((9, 1, 9, 'M > 8'), (8, 26, 33, 'P = M + K - 1 > 32')):
        Xb = np.zeros((1, K, T, F, M), np.complex64)
        Zb = np.zeros((1, K, T, F), np.complex64)
        mb = np.zeros((1, K, T, F), np.float32)
        eng = _engine(make_engine, 1, K, M, T, 512)
        try:
            rc, msg = raw_cov(eng, Xb, mb, Zb if K > 1 else None, Zb if K > 1 else None, P)
            assert rc == -2 and want in msg, (rc, msg)
        finally:
            eng.close()
    X, Zs, Zn, mask = scene(2, 1, 5, 5, T, F, True)                      # disco_step2_cov_fused with P = 9 > 8
    eng = _engine(make_engine, 1, 5, 5, T, 512)
    try:
        with _raises(eng, -2, 'M + K - 1 > 8'):
            eng.step2_cov_fused(X, mask, sparse_filters(1, 1, 5, F, 5))
        usable(eng, X, mask, Zs)                                         # k_cov_big on the same context
    finally:
        eng.close()


class _raises:
    def __init__(self, eng, rc, text):
        self.eng, self.rc, self.text = eng, rc, text

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None, f'no refusal (expected {self.rc}: {self.text})'
        assert f'error {self.rc}:' in str(ev) and self.text in str(ev), str(ev)
        return True


# ---- the solvers' loaders of the partial sums, and the re-use route --------------------------------------------------------------------

def pencil_dist(a, ref):
    """(R, K, F, P) against the reference -> (R, K, F): || a - ref || / || ref || per pencil."""
    a, ref = np.asarray(a, np.complex128), np.asarray(ref, np.complex128)
    return np.linalg.norm(a - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)


def solve_bar(Sss, Snn, T, mu=1.0, rounded=None):
    """-> w_ref, t1_ref (float64 oracle on the float64 means), the bars of w and of t1, each (R, K, F): per pencil, BAR_FACTOR x the
    distance from that reference of the same oracle fed `rounded` = the means in the kernels' number formats (default: the means
    rounded once to complex64, what an exact scene leaves; the re-use route passes the float32 restatement of its sums), never below
    SOLVE_FLOOR -- and the two raw distances.  Reference side only, recomputed on the inputs of every case (not a committed table).
    Per pencil, because the distance follows the pencil's conditioning: an exactly known scene now and then holds a pencil whose two
    largest eigenvalues nearly tie, and that one moves under any rounding."""
    a, b = Sss / T, Snn / T
    w, t1, _ = mo.gevd_mwf_r1_hermitian(a, b, mu)
    a32, b32 = (a.astype(np.complex64), b.astype(np.complex64)) if rounded is None else rounded
    assert a32.dtype == np.complex64 and b32.dtype == np.complex64
    w32, t32, _ = mo.gevd_mwf_r1_hermitian(a32, b32, mu)
    dw, dt = pencil_dist(w32, w), pencil_dist(t32, t1)
    return w, t1, np.maximum(SOLVE_FLOOR, BAR_FACTOR * dw), np.maximum(SOLVE_FLOOR, BAR_FACTOR * dt), dw, dt


def _check_solution(eng, P, ref, what, min_floor_share=0.9):
    """-> (worst distance of a pencil, the share of pencils held to the floor bar, the median reference-side distance)."""
    w_ref, t_ref, bar_w, bar_t, d_w, d_t = ref
    w, t1 = eng.gevd_mwf_r1_pending(P, want_t1=True)
    dw, dt = pencil_dist(w.numpy(), w_ref), pencil_dist(t1.numpy(), t_ref)
    bad_w, bad_t = ~(dw <= bar_w), ~(dt <= bar_t)
    assert not bad_w.any() and not bad_t.any(), (
        f'{what}: pending solve outside its per-pencil bar: w {_first_bad(bad_w)} (worst ratio {float((dw / bar_w).max()):.2f}); '
        f't1 {_first_bad(bad_t)} (worst ratio {float((dt / bar_t).max()):.2f})')
    at_floor = float(np.mean((bar_w == SOLVE_FLOOR) & (bar_t == SOLVE_FLOOR)))
    # the scene is well conditioned: (nearly) every pencil is held to the floor bar, so a wrong loader cannot hide behind loose bars
    assert at_floor > min_floor_share, f'{what}: test bug: only {at_floor:.2f} of the pencils are well conditioned'
    return float(max(dw.max(), dt.max())), at_floor, float(np.median(d_w))


PENDING_CHUNKS = (1, 2, 3, 5, 8)
T_PENDING = 61                                 # not a power of two, not divisible by 2, 3, 5 or 8: ragged chunks


# label: ((M, K, step2), options, the solver whose loader reads the partial blocks).  Which solver takes which P is api_solve.hip's rule
# (include/disco_hip.h, disco_set_option): P <= 4 and, by default, 5 .. 8 one thread per pencil (k_solve_small.h); 9 .. 16 the DPP
# solver (k_solve_dpp.h); 17 .. 32 one wave per pencil (k_solve_wide.h); with "solve_thread" = 0 (5 .. 8) or "solve_dpp" = 0 (9 .. 16)
# the LDS group solver (k_solve.h).  k_cov_loc_f64 leaves (hi, lo) pairs: 2 x chunks blocks.
PENDING = {
    'k_cov': ((2, 3, True), None, 'k_solve_small.h, P = 4'),
    'k_cov/P3': ((2, 2, True), None, 'k_solve_small.h, P = 3'),
    'k_cov_loc_f64': ((7, 1, False), None, 'k_solve_small.h, P = 7, 2 x chunks blocks'),
    'k_cov_loc_f64/group': ((7, 1, False), {'solve_thread': 0}, 'k_solve.h, P = 7, 2 x chunks blocks'),
    'k_cov/group': ((3, 4, True), {'solve_thread': 0}, 'k_solve.h, P = 6'),
    'k_cov_big': ((3, 8, True), None, 'k_solve_dpp.h, P = 10'),
    'k_cov_big/group': ((3, 8, True), {'solve_dpp': 0}, 'k_solve.h, P = 10'),
    'k_cov_split_lds': ((2, 8, True), None, 'k_solve_dpp.h, P = 9'),
    'k_cov_wide': ((2, 17, True), None, 'k_solve_wide.h, P = 18'),
    'k_step2_cov_fused': (FUSED_SHAPE + (True,), None, 'k_solve_small.h, P = 4'),
}


def check_pending(make_engine, T_all=T_PENDING, chunk_counts=PENDING_CHUNKS, families=None):
    """Every entry of PENDING x chunk count: covariance call with Rss = Rnn = NULL, then the pending solve, per pencil against the
    oracle.  The sums are exact, so the result must not depend on the chunk count at all (asserted bit for bit)."""
    out = {}
    for name, ((M, K, step2), options, loader) in PENDING.items():
        if families is not None and name not in families:
            continue
        fused = name == 'k_step2_cov_fused'
        F = 257
        P = M + (K - 1 if step2 else 0)
        T = max(T_all, 4 * P)                                            # enough frames for definite P x P matrices
        X, Zs, _zn, mask = scene(_seed(M, K, 9), 1, K, M, T, F, step2 and not fused, solvable=True)
        if fused:
            w_loc = sparse_filters(5, 1, K, F, M)
            Zs = np.einsum('rkfm,rktfm->rktf', w_loc.conj(), X).astype(np.complex64)
        Sss, Snn = ref_sums(X, mask, Zs, Zs)
        ref = solve_bar(Sss, Snn, T)
        eng = _engine(make_engine, 1, K, M, T, 512)
        try:
            for k_, v_ in (options or {}).items():
                eng.set_option(k_, v_)
            first = None
            for c in chunk_counts:
                if fused:
                    eng.set_tuning(step2_chunks=c)
                    px, kx = eng.to_device(X, np.complex64)
                    pm, km = eng.to_device(mask, np.float32)
                    pw, kw = eng.to_device(w_loc, np.complex64)
                    eng._chk(eng.lib.disco_step2_cov_fused(eng.ctx, px, pm, pw, None, None, None, eng.stream))
                else:
                    eng.set_tuning(cov_chunks=c)
                    eng.cov_masked(X, mask, Zs, Zs, Rss_out=False)
                res = _check_solution(eng, P, ref, f'{name} ({loader}) chunks={c}')
                first = res if first is None else first
                assert res == first, f'{name} ({loader}): the solution depends on the chunk count ({c}): {res} != {first}'
            out[name] = first + (loader,)
        finally:
            eng.close()
    return out


def check_reuse(make_engine, shapes=None, T=64, n_fft=512):
    """disco_step2_cov_fused_reuse (k_step2_cov_fused<M, K, true>) after disco_stft_cov_fused, as its contract says.  z_out is
    bit-identical to the non-reuse call's and is w_loc^H X (float64 product, one float32 rounding per product and sum).  Its pending
    solve -- the one solve that assembles a pencil from TWO sets of partial blocks -- is compared per pencil with the float64 oracle on
    the float64 covariance of the spectra X the library returned and the float64 z = w_loc^H X.  The sums of this route are float32
    accumulations, so the reference-side perturbation behind the bar is `cov_f32_restatement` of the same inputs (all T frames in one
    run: the longest float32 sum any chunking makes) in place of one rounding of the means; the rule is otherwise solve_bar's."""
    shapes = reuse_shapes() if shapes is None else shapes
    out = {}
    for M, K in shapes:
        rng = np.random.default_rng(_seed(M, K, 13))
        eng = _engine(make_engine, 1, K, M, T, n_fft)
        try:
            P = M + K - 1
            y, mask_h = bursty_clip(rng, K, M, eng.Lsamp, T, eng.F, HOP[n_fft])
            pm, mask = eng.to_device(mask_h, np.float32)                  # the re-use is granted for THE arrays step 1 saw
            X, _a, _b2 = eng.stft_cov_fused(y, mask, want_cov=False)
            w_loc, _t = eng.gevd_mwf_r1_pending(M)
            z = eng.step2_cov_fused_reuse(X, mask, w_loc, want_z=True).numpy()
            what = f'k_step2_cov_fused<{M},{K},true>'
            Xh, wl = X.numpy(), w_loc.numpy().astype(np.complex128)
            z_ref = np.einsum('rkfm,rktfm->rktf', wl.conj(), Xh.astype(np.complex128))
            rs, rn = float_ref(Xh, z_ref, mask_h, spread=None)
            ref = solve_bar(rs, rn, 1, rounded=tuple(cov_f32_restatement(Xh, z_ref.astype(np.complex64), mask_h)))
            out[(M, K)] = _check_solution(eng, P, ref, what, min_floor_share=0.0)
            _r1, _r2, z2 = eng.step2_cov_fused(X, mask, w_loc, want_z=True)
            assert np.array_equal(_bits(z), _bits(z2.numpy())), f'{what}: z_out differs from the non-reuse call'
            scale = np.einsum('rkfm,rktfm->rktf', np.abs(wl.real) + np.abs(wl.imag), np.abs(Xh.real) + np.abs(Xh.imag).astype(np.float64))
            bad = ~(np.abs(z - z_ref) <= 2 * M * 2.0 ** -24 * scale)     # 2 M products and sums per part, each rounded once
            assert not bad.any(), f'{what}: z_out is not w_loc^H X: {_first_bad(bad.any(axis=2))}'
        finally:
            eng.close()
    return out


def bursty_clip(rng, K, M, L, T, F, hop):
    """One room of time signals y (1, K, M, L) f32 -- one white source, on or off per hop, delayed and scaled per channel, plus white
    noise of unit variance -- and masks (1, K, T, F) that follow the source (3/4 or 1 where it is on, 1/4 or 1/2 where it is off):
    well-conditioned step-1 pencils with a clear top eigenvalue."""
    on = rng.integers(0, 2, T + 1).astype(np.float64)
    on[:2] = (1.0, 0.0)
    gate = np.repeat(on, hop)[hop // 2:hop // 2 + L + 64]
    src = 2.0 * rng.standard_normal(L + 64) * gate
    y = np.empty((1, K, M, L), np.float32)
    for k in range(K):
        for m in range(M):
            d = int(rng.integers(0, 64))
            y[0, k, m] = (rng.uniform(0.7, 1.4) * rng.choice((-1.0, 1.0)) * src[d:d + L] + rng.standard_normal(L)).astype(np.float32)
    a = np.broadcast_to(on[None, None, :T, None], (1, K, T, F))
    mask = MASK_VALUES[np.where(a == 1, rng.integers(3, 5, (1, K, T, F)), rng.integers(1, 3, (1, K, T, F)))]
    return y, np.ascontiguousarray(mask.astype(np.float32))


# ---- the float tier: float32 accumulation at the production chunk length ---------------------------------------------------------------
# On the exact scenes nothing rounds.  Here the staged families run the unit-variance Gaussian scene of parity_checks._rand_stft_scene at
# T = 626 frames in ONE chunk -- what a large batch runs -- where every float32 accumulator rounds 626 times.  Two quantities per pencil:
#     fro = || R - ref ||_F / || ref ||_F
#     coh = max_ij | R_ij - ref_ij | / sqrt(ref_ii ref_jj)        (one wrong small entry is not averaged away)
# against the float64 covariance of the same complex64 inputs.  THE BAR is measured on the reference side alone: `cov_f32_restatement`
# (NumPy, no kernel code) applies the masks in float32, accumulates the frames of a chunk one after the other in float32, adds the chunks
# in float64 and rounds the mean as the library does; FLOAT_DIST holds its worst per-pencil distance from the float64 reference on the
# very inputs of the check, per family (= per P) and quantity, times 1.1 and rounded up to two digits.  A kernel passes within
# BAR_FACTOR = 4 times that, the factor of tests/online_checks.py and for its two reasons: the kernel and the restatement are two
# independent float32 roundings of one sum (x 2), times 2 for the spread between seeds.  tests/test_cov_routes_cpu.py recomputes the
# table and holds the committed figures inside [1, 2] x what it finds.  k_cov_loc_f64 accumulates in float64 and sits far inside.

T_FLOAT = 626
FLOAT_SHAPES = {                               # family: (M, K, step2)
    'k_cov': (2, 3, True),
    'k_cov_loc_f64': (7, 1, False),
    'k_cov_big': (3, 8, True),
    'k_cov_split_lds': (2, 8, True),
    'k_cov_wide': (8, 10, True),
}
FLOAT_DIST = {                                 # family: (fro, coh) of the restatement, T = 626 in one chunk
    'k_cov': (1.4e-06, 1.7e-06),
    'k_cov_loc_f64': (7.5e-07, 1.6e-06),
    'k_cov_big': (1.1e-06, 1.9e-06),
    'k_cov_split_lds': (1.2e-06, 1.8e-06),
    'k_cov_wide': (7.7e-07, 1.9e-06),
}


def round_up(x):
    """x * 1.1 rounded up to two significant digits."""
    x = x * 1.1
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


def float_scene(family, T=T_FLOAT, F=257):
    import zlib
    from parity_checks import _rand_stft_scene
    M, K, step2 = FLOAT_SHAPES[family]
    rng = np.random.default_rng(zlib.crc32(family.encode()))
    X, mask = _rand_stft_scene(rng, 1, K, M, T, F)
    Z = None
    if step2:
        Z = ((rng.standard_normal((1, K, T, F)) + 1j * rng.standard_normal((1, K, T, F))) / np.sqrt(2.0)).astype(np.complex64)
    return X, Z, mask


def float_ref(X, Z, mask, frames=None, spread=100.0):
    """float64 means (R, K, F, P, P) of the inputs (same z, mask_remote = 1; room r over its own frames[r]), and the scene's own
    property (spread: None skips it): every bin of every channel carries comparable energy, so that no pencil is all rounding."""
    R, K, T, F, M = X.shape
    P = M + (K - 1 if Z is not None else 0)
    Rss = np.zeros((R, K, F, P, P), np.complex128)
    Rnn = np.zeros_like(Rss)
    for r in range(R):
        Tr = T if frames is None else int(frames[r])
        for k in range(K):
            v = rows_of(X, Z, r, k, k)[:Tr]
            m = mask[r, k, :Tr].astype(np.float64)[..., None]
            vs = np.ascontiguousarray((m * v).transpose(1, 2, 0))
            vn = np.ascontiguousarray(((1 - m) * v).transpose(1, 2, 0))
            Rss[r, k] = vs @ vs.conj().transpose(0, 2, 1) / Tr
            Rnn[r, k] = vn @ vn.conj().transpose(0, 2, 1) / Tr
    if spread is not None:
        for A in (Rss, Rnn):
            d = np.einsum('...ii->...i', A).real
            assert d.min() > 0 and d.max() / d.min() < spread, (d.min(), d.max())
    return Rss, Rnn


def cov_f32_restatement(X, Z, mask, chunks=1, chunk_frames=None, frames=None):
    """The covariance in the kernels' number formats, NumPy only: masks applied in float32, the frames of a chunk accumulated one after
    the other in float32 (complex64 products and sums), chunks added in float64, the mean float32(S * float64(float32(1) / float32(T))).
    chunks: that many chunks [T c / chunks, T (c + 1) / chunks); chunk_frames: chunks of that many frames instead; frames: per-room T_r."""
    R, K, T, F, M = X.shape
    P = M + (K - 1 if Z is not None else 0)
    out = []
    for comp in (False, True):
        A = np.zeros((R, K, F, P, P), np.complex64)
        for r in range(R):
            Tr = T if frames is None else int(frames[r])
            it = np.float64(np.float32(1) / np.float32(Tr))
            if chunk_frames:
                bounds = [(t, min(t + chunk_frames, Tr)) for t in range(0, Tr, chunk_frames)]
            else:
                bounds = [(Tr * c // chunks, Tr * (c + 1) // chunks) for c in range(chunks)]
            for k in range(K):
                v = rows_of(X, Z, r, k, k).astype(np.complex64)                      # (T, F, P)
                m = mask[r, k].astype(np.float32)[..., None]
                v = ((np.float32(1) - m) if comp else m) * v
                assert v.dtype == np.complex64
                tot = np.zeros((F, P, P), np.complex128)
                for t0, t1 in bounds:
                    acc = np.zeros((F, P, P), np.complex64)
                    for t in range(t0, t1):
                        acc += v[t][:, :, None] * np.conjugate(v[t])[:, None, :]
                    assert acc.dtype == np.complex64
                    tot += acc
                A[r, k] = (tot.real * it).astype(np.float32) + 1j * (tot.imag * it).astype(np.float32)
        out.append(A)
    return out


def pencil_quantities(A, ref):
    """-> fro, coh, each (R, K, F)."""
    A = np.asarray(A, np.complex128)
    fro = np.linalg.norm(A - ref, axis=(-1, -2)) / np.linalg.norm(ref, axis=(-1, -2))
    d = np.sqrt(np.einsum('...ii->...i', ref).real)
    coh = (np.abs(A - ref) / (d[..., :, None] * d[..., None, :])).max(axis=(-1, -2))
    return fro, coh


def recompute_float_dist(families=None):
    found = {}
    for fam in (FLOAT_SHAPES if families is None else families):
        X, Z, mask = float_scene(fam)
        rs, rn = float_ref(X, Z, mask)
        a, b = cov_f32_restatement(X, Z, mask)
        qa, qb = pencil_quantities(a, rs), pencil_quantities(b, rn)
        found[fam] = (float(max(qa[0].max(), qb[0].max())), float(max(qa[1].max(), qb[1].max())))
    return found


def check_float(make_engine, families=None, T=T_FLOAT):
    """Every staged family on the Gaussian scene at T frames in one chunk, per pencil inside BAR_FACTOR x FLOAT_DIST (T = 626); a cut
    run (the emulator) measures the restatement's distance on its own inputs, with the same factor."""
    out = {}
    for fam in (FLOAT_SHAPES if families is None else families):
        M, K, step2 = FLOAT_SHAPES[fam]
        X, Z, mask = float_scene(fam, T)
        rs, rn = float_ref(X, Z, mask)
        if T == T_FLOAT:
            dist = FLOAT_DIST[fam]
        else:
            a, b = cov_f32_restatement(X, Z, mask)
            qa, qb = pencil_quantities(a, rs), pencil_quantities(b, rn)
            dist = (float(max(qa[0].max(), qb[0].max())), float(max(qa[1].max(), qb[1].max())))
        eng = _engine(make_engine, 1, K, M, T, 512)
        try:
            eng.set_tuning(cov_chunks=1)
            Rss, Rnn = eng.cov_masked(X, mask, Z, Z)
            worst = [0.0, 0.0]
            for got, ref, nm in ((Rss.numpy(), rs, 'Rss'), (Rnn.numpy(), rn, 'Rnn')):
                for i, (q, qn) in enumerate(zip(pencil_quantities(got, ref), ('fro', 'coh'))):
                    bar = BAR_FACTOR * dist[i]
                    assert not (~(q <= bar)).any(), f'{fam} {nm} {qn}: worst {float(q.max()):.3e}, bar {bar:.3e}: {_first_bad(~(q <= bar))}'
                    worst[i] = max(worst[i], float(q.max()))
            out[fam] = {'fro': worst[0], 'coh': worst[1], 'bar_fro': BAR_FACTOR * dist[0], 'bar_coh': BAR_FACTOR * dist[1]}
        finally:
            eng.close()
    return out


# ---- the float tier of disco_stft_cov_fused: a transform is in the way of exactness -----------------------------------------------------
# Compared end to end with float64: oracle/stft_oracle.py in complex128 on the samples, then the float64 covariance -- not with the
# covariance of the device's own spectra.  Same two per-pencil quantities and the same rule for the bar: STFT_DIST holds, per case, the
# worst per-pencil distance from that reference of the NumPy restatement (the float64 spectra rounded once to complex64, masks applied
# in float32, the frames of a workgroup's chunk -- 4 waves x stft_frames_per_wave -- accumulated one after the other in float32, chunks
# added in float64, the mean rounded as the library does), times 1.1 and rounded up; a kernel passes within BAR_FACTOR times that.
# White Gaussian samples keep every bin's energy comparable (asserted on the reference), so the transform's float32 floor dominates no bin.

STFT_WAVES = 4                                 # waves of a k_stft_cov workgroup (k_stft.h)
STFT_RUN_DEFAULT = 8                           # what stft_cov_chunks picks for the small batches here: max(8, T / (4 x many chunks))


def stft_cases():
    """id -> dict(M, n_fft, pad, T, runw (0: heuristic), frames (per-room T_r or None))."""
    c = {}
    for M in range(1, 9):                                                # every k_stft_cov<512, M>; both pad modes alternate
        c[f'512-M{M}'] = dict(M=M, n_fft=512, pad='reflect' if M % 2 else 'constant', T=63, runw=0, frames=None)
    for M in range(1, 9):                                                # k_stft_cov<1024, M <= 6>; M = 7, 8: k_stft + k_cov_loc_f64
        c[f'1024-M{M}'] = dict(M=M, n_fft=1024, pad='constant' if M % 2 else 'reflect', T=63, runw=0, frames=None)
    for runw in (8, 40, 79, 80, 400):                                    # 400 > T: one wave holds the clip, three are empty
        c[f'run{runw}'] = dict(M=4, n_fft=512, pad='reflect', T=330, runw=runw, frames=None)
    c['empty-waves'] = dict(M=3, n_fft=512, pad='reflect', T=100, runw=8, frames=None)       # 100 = 3 x 32 + 4: the last workgroup has 4 frames
    c['T2'] = dict(M=2, n_fft=512, pad='constant', T=2, runw=0, frames=None)
    c['T3'] = dict(M=2, n_fft=512, pad='reflect', T=3, runw=0, frames=None)
    c['T3-1024'] = dict(M=5, n_fft=1024, pad='constant', T=3, runw=0, frames=None)
    c['lengths-512'] = dict(M=4, n_fft=512, pad='reflect', T=63, runw=0, frames=(63, 37))
    c['lengths-run40'] = dict(M=3, n_fft=1024, pad='constant', T=100, runw=40, frames=(20, 100))
    c['lengths-staged'] = dict(M=7, n_fft=1024, pad='reflect', T=63, runw=0, frames=(41, 63))
    return c


STFT_DIST = {                                  # id: (fro, coh) of the restatement
    '512-M1': (2.7e-07, 2.7e-07),
    '512-M2': (3.4e-07, 3.9e-07),
    '512-M3': (2.4e-07, 3.7e-07),
    '512-M4': (2.4e-07, 3.5e-07),
    '512-M5': (2e-07, 3.3e-07),
    '512-M6': (1.9e-07, 3.4e-07),
    '512-M7': (2.1e-07, 3.3e-07),
    '512-M8': (1.8e-07, 3.6e-07),
    '1024-M1': (3e-07, 3e-07),
    '1024-M2': (2.6e-07, 3.2e-07),
    '1024-M3': (2.6e-07, 3.4e-07),
    '1024-M4': (2.3e-07, 3.8e-07),
    '1024-M5': (2.2e-07, 3.7e-07),
    '1024-M6': (2.2e-07, 3.7e-07),
    '1024-M7': (3.2e-07, 5.6e-07),
    '1024-M8': (3.2e-07, 6e-07),
    'run8': (1.1e-07, 1.8e-07),
    'run40': (3.3e-07, 5.8e-07),
    'run79': (6.5e-07, 1.1e-06),
    'run80': (5.9e-07, 9.9e-07),
    'run400': (6.9e-07, 1.2e-06),
    'empty-waves': (1.9e-07, 3.1e-07),
    'T2': (2.7e-07, 3.2e-07),
    'T3': (2.5e-07, 2.9e-07),
    'T3-1024': (2.4e-07, 3.4e-07),
    'lengths-512': (2.8e-07, 4.1e-07),
    'lengths-run40': (5.4e-07, 8.5e-07),
    'lengths-staged': (3.3e-07, 6e-07),
}


def stft_scene(cid, case, K=2):
    """-> y (R, K, M, L) f32 white Gaussian, mask (R, K, T, F) f32, lengths (R,) or None, and the float64 side: X (R, K, T, F, M)
    complex128 from oracle/stft_oracle.py on every room's own samples (zeros beyond its frames)."""
    import zlib
    from oracle import stft_oracle as so
    n_fft, T, M = case['n_fft'], case['T'], case['M']
    hop, F = HOP[n_fft], n_fft // 2 + 1
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    R = 1 if case['frames'] is None else len(case['frames'])
    L = (T - 1) * hop + 17
    y = rng.standard_normal((R, K, M, L)).astype(np.float32)
    mask = rng.uniform(0.05, 0.95, (R, K, T, F)).astype(np.float32)
    lengths = None if case['frames'] is None else [(t - 1) * hop + 5 for t in case['frames']]
    X = np.zeros((R, K, T, F, M), np.complex128)
    for r in range(R):
        Lr = L if lengths is None else lengths[r]
        S = so.stft(y[r, :, :, :Lr].astype(np.float64), n_fft, hop, case['pad'], np.complex128)            # (K, M, F, T_r)
        X[r, :, :S.shape[-1]] = S.transpose(0, 3, 2, 1)
        assert S.shape[-1] == (T if case['frames'] is None else case['frames'][r])
    return y, mask, lengths, X


def stft_chunk_frames(case):
    if case['n_fft'] == 1024 and case['M'] > 6:
        return None                                                     # the staged pair: k_cov_loc_f64, float64 accumulators (one run here)
    return STFT_WAVES * (case['runw'] or STFT_RUN_DEFAULT)


def stft_reference(cid, case):
    """-> y, mask, lengths, the float64 means (Rss, Rnn) and the restatement's distances (fro, coh)."""
    y, mask, lengths, X = stft_scene(cid, case)
    rs, rn = float_ref(X, None, mask, frames=case['frames'], spread=100.0 if case['T'] >= 63 else None)
    a, b = cov_f32_restatement(X.astype(np.complex64), None, mask, chunk_frames=stft_chunk_frames(case), frames=case['frames'])
    qa, qb = pencil_quantities(a, rs), pencil_quantities(b, rn)
    return y, mask, lengths, rs, rn, (float(max(qa[0].max(), qb[0].max())), float(max(qa[1].max(), qb[1].max())))


def recompute_stft_dist(ids=None):
    return {cid: stft_reference(cid, case)[5] for cid, case in stft_cases().items() if ids is None or cid in ids}


def check_stft_cov(make_engine, ids=None):
    """disco_stft_cov_fused, every case of stft_cases (or `ids`), per pencil inside BAR_FACTOR x STFT_DIST."""
    out = {}
    for cid, case in stft_cases().items():
        if ids is not None and cid not in ids:
            continue
        y, mask, lengths, rs, rn, _d = stft_reference(cid, case)
        dist = STFT_DIST[cid]
        R, K, M, L = y.shape
        eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=case['n_fft'], pad_mode=case['pad'])
        try:
            assert eng.T == case['T']
            if case['runw']:
                eng.set_tuning(stft_frames_per_wave=case['runw'])
            if lengths is not None:
                eng.set_lengths(lengths)
                assert tuple(eng.frames) == tuple(case['frames'])
            _X, Rss, Rnn = eng.stft_cov_fused(y, mask)
            worst = [0.0, 0.0]
            for got, ref, nm in ((Rss.numpy(), rs, 'Rss'), (Rnn.numpy(), rn, 'Rnn')):
                for i, (q, qn) in enumerate(zip(pencil_quantities(got, ref), ('fro', 'coh'))):
                    bar = BAR_FACTOR * dist[i]
                    assert not (~(q <= bar)).any(), (f'disco_stft_cov_fused {cid} {route(M, 1, case["n_fft"], False, call="stft_cov")} {nm} {qn}: '
                                                     f'worst {float(q.max()):.3e}, bar {bar:.3e}: {_first_bad(~(q <= bar))}')
                    worst[i] = max(worst[i], float(q.max()))
            out[cid] = {'fro': worst[0], 'coh': worst[1], 'bar_fro': BAR_FACTOR * dist[0], 'bar_coh': BAR_FACTOR * dist[1]}
        finally:
            eng.close()
    return out


# ---- more than 2^31 elements in X: the 64-bit offsets -----------------------------------------------------------------------------------

HUGE = {'k_cov': (4, 4, False, 840), 'k_cov_big': (3, 8, True, 560)}      # family: (M, K, step2, rooms): rooms x K x 626 x 257 x M > 2^31


def check_huge(make_engine, device, rooms=None, T=626):
    """X beyond 2^31 complex elements (17 GB), generated on the device with torch as exact inputs (integer parts in [-2, 2], masks from
    MASK_VALUES, integer z); the heuristic runs all 626 frames in one chunk.  The first and the last room are brought to the host and
    compared exactly, every node and bin: a 32-bit offset anywhere lands the last room's units on other rooms' data."""
    import torch
    out = {}
    for name, (M, K, step2, R) in HUGE.items():
        R = R if rooms is None else rooms
        F = 257
        if rooms is None:
            assert R * K * T * F * M > 2 ** 31
        g = torch.Generator(device=device)
        g.manual_seed(_seed(M, K, 17))

        def ints(*shape):
            return torch.view_as_complex(torch.randint(-2, 3, shape + (2,), device=device, generator=g, dtype=torch.int8).to(torch.float32))
        X = ints(R, K, T, F, M)
        Z = ints(R, K, T, F) if step2 else None
        mask = torch.randint(0, 5, (R, K, T, F), device=device, generator=g, dtype=torch.int8).to(torch.float32) / 4
        if device != 'cpu':
            torch.cuda.synchronize()
        eng = _engine(make_engine, R, K, M, T, 512)
        try:
            Rss, Rnn = eng.cov_masked(X, mask, Z, Z)
            ends = [0, R - 1]
            Xh, mh = X[ends].cpu().numpy(), mask[ends].cpu().numpy()
            Zh = Z[ends].cpu().numpy() if step2 else None
            Sss, Snn = ref_sums(Xh, mh, Zh, Zh)
            what = f'{route(M, K, 512, step2)[0]} with {R * K * T * F * M} elements in X, rooms 0 and {R - 1}'
            compare_exact(Rss.numpy()[ends], Sss, [T, T], what + ' Rss')
            compare_exact(Rnn.numpy()[ends], Snn, [T, T], what + ' Rnn')
            out[name] = R * K * T * F * M
        finally:
            eng.close()
        del X, Z, mask
    return out
