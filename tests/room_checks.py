"""Checks, pencil by pencil, of the three producers of a TAIL-BLOCK pencil -- a pencil the solver assembles from the kept step-1 sums plus
a second set of partial blocks:
    k_room_cov_dma<M, K, 8>        csrc/k_room.h, the persistent one-pass room kernel (option "room_cov" = 1)
    k_cov_split_lds<M, KR, true>   csrc/k_cov.h, the staged wide route with the leading M x M block skipped ("room_cov" = 0)
    k_step2_cov_fused<M, K, true>  csrc/k_fused.h, the re-use route of the fused step 2
The first two run from the caller's spectra through the test-only entry disco_selftest_staged_step2 (step 1 on X, then the very host
function the whole-path calls run), the third through disco_cov_masked(P = M) + disco_step2_cov_fused_reuse; the matrices of the pending
pencil come from disco_selftest_pending_matrices (include/disco_hip.h).

Shared by tests/test_gpu_room_routes.py (real MI355X, `-m gpu`), tests/test_room_routes_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut down) and tests/test_cov_routes_cpu.py (the reference side: tables against the headers, coverage of the cases).
Every helper of the exact tier is tests/cov_checks.py's: the scenes, `ref_sums` with its 2^24 bound, `compare_exact` (the rules at the
top of that file: equal to S / T bit for bit when T is a power of two, inside MEAN_TOL per component otherwise, exact zeros, conjugate
symmetry, real diagonals, per (room, node, bin), no bin excluded), `solve_bar` / `_check_solution` for the pending solves.

THE EXACT TIER here: integer spectra, masks from {0, 1/4, 1/2, 3/4, 1} and filters w_loc with two or three taps from {+-1, +-i, +-1 +- i}
(`room_filters`), so z = w_loc^H X is a small Gaussian integer and must come back bit for bit, and every sum -- the eight sub-chunk sums
of the room pass, their float64 meeting, the (hi, lo) split -- is exact.  Then
    * the matrices obey the rules above and their leading M x M block is bit-identical to what disco_cov_masked(X, mask, P = M) hands out;
    * where every room has T_r >= 4 P frames the pending solve is held per pencil to solve_bar's rule under "solve_dpp" 0 and 1 (the two
      loaders of a two-block pencil of 9 <= P <= 16: k_solve.h and k_solve_dpp.h);
    * route_out and the stage names say which kernel ran.

Per-room lengths: the covariance kernels of csrc/k_cov.h cut every chunk at the room's own frame count (cov_chunk_frames) and the room
pass neither fetches nor weighs a frame beyond it and writes z = 0 there, so what X and the mask hold beyond T_r does not matter to
them: `check_nan_beyond` puts NaN there, in both, and no output bit may change.  disco_apply (the z of the split route) knows no
lengths and relies on the zeros the library's own spectra hold there: `check_staged` zeroes X beyond T_r and fills the MASK with finite
garbage on both routes.

THE FLOAT TIER (`check_float`): the Gaussian scene of parity_checks._rand_stft_scene at 626 frames, random filters of unit expected norm,
per pencil fro and coh against the float64 covariance exactly as cov_checks.check_float; the bar is BAR_FACTOR x the distance of
cov_checks.cov_f32_restatement of the same inputs (all frames in one float32 run), measured on the reference side on every run.
    Worst measured per route: FLOAT_MEASURED below (MI355X), next to the bars they were held to.  The room pass sums an eighth of the
    frames per accumulator and meets in float64: on (8, 8), where step 1 accumulates in float64 too, it sits 25 times inside the bar.
"""
import numpy as np

import cov_checks as cc
from cov_checks import HOP, _bits, _engine, _first_bad, _seed

ROOM = cc.ROOM                                                                         # DISCO_FOR_ROOM (dispatch.h): (M, K)
SPLIT_SHAPES = tuple((M, KR + 1) for M, KR in cc.SPLIT if KR > 0)                      # (M, K) of k_cov_split_lds<M, KR, true>: 24
ROOM_SUB, ROOM_DEPTH = 8, 6                                                            # frames per group, ring slots (k_room.h)
# frame counts around the ring of the room pass: 8 frames per sub-chunk group, two groups per iteration (16), six slots (48), loads two
# iterations ahead (32)
RING_T = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49)
RING_T_SUBSET = (1, 9, 16, 33)
RING_T_CUT = (2, 9, 17)
# (T, cov_chunks) of the split route: chunk c covers frames [T c / chunks, T (c + 1) / chunks) -- frame counts either side of the chunk
# boundaries (15 | 16 | 17 in two chunks: 7 + 8, 8 + 8, 8 + 9; 31 | 32 | 33 in four), fewer frames than chunks, one frame, the heuristic
SPLIT_GEOMETRY = ((15, 2), (16, 2), (17, 2), (31, 4), (32, 4), (33, 4), (2, 8), (1, 0), (9, 0), (49, 3))
# the float tier as measured on an MI355X (T = 626, one room): worst per-pencil (fro, coh) by (M, K, route), and the bars (fro, coh) the
# run held them to = BAR_FACTOR x the restatement's distance on the same inputs.  A record, not a bound: check_float measures its bar anew.
# The pending solves of the exact tier on the same device: worst per-pencil distance from the float64 oracle 4.6e-8 (room pass and split
# route, identical under "solve_dpp" 0 and 1) and 5.2e-8 (re-use route) against bars of at least 2e-6: ratios <= 0.026; between 0.80 and
# 1.00 of the pencils of a scene are held to that floor bar.
FLOAT_MEASURED = {
    (8, 8, 'room'): ((9.8e-08, 2.2e-07), (2.5e-06, 6.5e-06)),
    (8, 8, 'split_skiploc'): ((5.7e-07, 1.4e-06), (2.5e-06, 6.5e-06)),
    (4, 6, 'room'): ((7.2e-07, 2.2e-06), (2.8e-06, 5.8e-06)),
    (4, 6, 'split_skiploc'): ((7.7e-07, 2.2e-06), (2.8e-06, 5.8e-06)),
}

# share of the pencils of a solvable scene that must be held to the 2e-6 floor bar (a property of the scene, asserted on the reference
# side): cov_checks asks 0.9 of its scenes of >= 61 frames; the frame counts here stop at 49, as few as 4 P frames per pencil, where the
# top eigenvalue stands less clear: three pencils in four
FLOOR_SHARE = 0.75
ROUTE_STAGES = {'room': {'room_cov2'}, 'split_skiploc': {'apply1', 'cov2'}, 'whole': {'apply1', 'cov2'}}


def expected_route(M, K, room_cov):
    """What disco_selftest_staged_step2 reports (api_path.hip staged_step2, api_room.hip room_cov_ok, api_cov.hip cov_partials)."""
    if room_cov and (M, K) in ROOM and M + K - 1 > 8:
        return 'room'
    if K > 1 and (M, K - 1) in cc.SPLIT and 8 < M + K - 1 <= cc.CB_PMAX:
        return 'split_skiploc'
    return 'whole'


def kernel_of(M, K, n_fft, room_cov):
    """The covariance kernel behind a staged-step-2 call, in the form cov_checks.route writes names."""
    r = expected_route(M, K, room_cov)
    if r == 'room':
        return f'k_room_cov_dma<{M},{K},{ROOM_SUB}>'
    if r == 'split_skiploc':
        return f'k_cov_split_lds<{M},{K - 1},true>'
    return cc.route(M, K, n_fft, True)[0]


# ---- the list of cases ----------------------------------------------------------------------------------------------------------------

def staged_cases(cut=False):
    """dicts of keyword arguments of `check_staged`.  cut: the emulator's list."""
    cases = []

    def add(M, K, n_fft=512, T=17, R=1, room_cov=1, **kw):
        c = dict(M=M, K=K, n_fft=n_fft, T=T, R=R, room_cov=room_cov, **kw)
        if c not in cases:
            cases.append(c)
    if cut:
        for T in RING_T_CUT:                                               # (8, 2) and (4, 6) at 512 points, three frame counts
            add(8, 2, T=T)
            add(4, 6, T=T)
        add(4, 6, T=37)                                                    # T >= 4 P: the pending solves
        add(8, 2, 1024, T=9)                                               # one 1024-point room case
        add(8, 2, T=9, R=3, frames=(9, 1, 6))                              # one mixed-length batch: a one-frame room next to a full one
        add(8, 2, T=9, store_z=False)
        for M, K, T, ch in ((8, 3, 9, 2), (4, 6, 41, 3), (2, 8, 9, 2)):    # one split shape per M
            add(M, K, T=T, room_cov=0, chunks=ch)
        return cases
    for M, K in ROOM:                                                      # the room pass: all six shapes at 512 and at 1024 points
        for n_fft in (512, 1024):
            for T in (RING_T if (M, K) in ((8, 2), (4, 6)) and n_fft == 512 else RING_T_SUBSET):
                add(M, K, n_fft, T=T)
    add(8, 2, T=37)                                                        # T >= 4 P (P = 9): the pending solves under both loaders
    add(4, 6, T=49)
    add(8, 4, T=45)                                                        # P = 11
    add(4, 8, 1024, T=47)
    # item walking: rooms x 65 tiles (512 points) over min(items, CUs) workgroups, rounded down to a multiple of 64: on 256 CUs R = 1, 2
    # and 8 make a workgroup walk one or two, two, and up to three items
    for R in (2, 8):
        add(8, 2, T=17, R=R)
        add(4, 6, T=9, R=R)
    add(8, 8, T=17, R=8)                                                   # the largest: 18 MB of spectra
    add(8, 8, 1024, T=9, R=2)
    add(8, 2, T=17, R=8, frames=(17, 1, 9, 16, 17, 8, 2, 15))              # consecutive items of a workgroup differ in frame count
    add(4, 6, T=33, R=8, frames=(33, 32, 1, 33, 17, 31, 16, 2))
    add(8, 6, T=17, R=2, frames=(1, 17))
    add(4, 8, 1024, T=16, R=3, frames=(16, 1, 9))
    add(8, 2, T=17, store_z=False)
    add(4, 6, T=33, R=2, store_z=False)
    add(8, 8, 1024, T=9, store_z=False)
    for M, K in SPLIT_SHAPES:                                              # the split route: all 24 shapes
        add(M, K, T=17 if M + K - 1 > 12 else 49, room_cov=0)
    add(8, 2, 1024, T=37, room_cov=0)
    add(4, 13, 1024, T=9, room_cov=0)
    add(2, 8, 1024, T=16, room_cov=0)
    for T, ch in SPLIT_GEOMETRY:
        add(8, 2, T=T, room_cov=0, chunks=ch)
        add(4, 6, T=T, room_cov=0, chunks=ch)
        add(2, 9, T=T, room_cov=0, chunks=ch)
    add(8, 2, T=17, R=8, room_cov=0, chunks=4, frames=(17, 1, 9, 16, 17, 8, 2, 15))
    add(4, 6, T=33, R=3, room_cov=0, chunks=2, frames=(33, 1, 17))
    add(8, 8, T=17, room_cov=0)                                            # room shapes with the room pass switched off
    return cases


def case_id(c):
    s = f"M{c['M']}K{c['K']}-{c['n_fft']}-T{c['T']}-R{c['R']}-{'room' if c['room_cov'] else 'staged'}"
    if c.get('frames'):
        s += '-lengths'
    if c.get('chunks'):
        s += f"-c{c['chunks']}"
    if c.get('store_z') is False:
        s += '-noz'
    return s


def launched_by(cases):
    return {kernel_of(c['M'], c['K'], c['n_fft'], c['room_cov']) for c in cases}


def reuse_cases(cut=False):
    """(M, K, T) of the exact re-use route: every shape of cov_checks.reuse_shapes; T alternates between a power of two and not, always
    >= 4 P (P <= 8) so that every shape's pending solve is checked too."""
    if cut:
        return [(2, 3, 32), (7, 2, 33)]
    return [(M, K, 32 if (M + K) % 2 else 37) for M, K in cc.reuse_shapes()]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

TAPS = np.array([1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j], np.complex64)


def room_filters(seed, R, K, F, M):
    """w_loc (R, K, F, M) with two or three non-zero taps from {+-1, +-i, +-1 +- i} per filter (fewer where M is smaller or two draws
    meet): z = w^H x stays a small Gaussian integer."""
    rng = np.random.default_rng(seed)
    w = np.zeros((R, K, F, M), np.complex64)
    idx = np.indices((R, K, F))
    n_taps = rng.integers(2, 4, (R, K, F))
    for i in range(3):
        m = rng.integers(0, M, (R, K, F))
        v = TAPS[rng.integers(0, 8, (R, K, F))]
        keep = i < n_taps
        w[idx[0][keep], idx[1][keep], idx[2][keep], m[keep]] = v[keep]
    return w


def exact_z(X, w_loc):
    """float64 w_loc^H X (R, K, T, F) -- exact: small integers."""
    return np.einsum('rkfm,rktfm->rktf', w_loc.conj().astype(np.complex128), X.astype(np.complex128))


def _lengths_of(frames, n_fft):
    return [(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in frames]


def _pencil_bits_equal(a, b):
    """(R, K, F, P, P) complex64 x 2 -> (R, K, F) bool: bit equality of whole pencils."""
    return (_bits(a).reshape(a.shape + (2,)) == _bits(b).reshape(b.shape + (2,))).all(axis=(-1, -2, -3))


def _run(eng, Xd, md, wd, P, store_z=True, z=None, want_stages=None):
    """One staged step 2 + the matrices of its pencil -> z (NumPy), route, Rss, Rnn (NumPy)."""
    if want_stages is not None:
        eng.stage_timing(True)
    zd, route = eng.selftest_staged_step2(Xd, md, wd, store_z=store_z, z=z)
    if want_stages is not None:
        stages = set(eng.stage_report())
        eng.stage_timing(False)
        assert stages == want_stages, (stages, want_stages)
    Rss, Rnn = eng.selftest_pending_matrices(P)
    return zd.numpy(), route, Rss, Rnn


Z_PATTERN = 0x7FC5A5A5                                                    # a NaN payload no kernel would write


def _pattern_z(eng, shape):
    pat = np.full(shape + (2,), Z_PATTERN, np.uint32).view(np.float32).view(np.complex64).reshape(shape)
    _p, buf = eng.to_device(pat, np.complex64)
    return buf


def check_staged(make_engine, M, K, n_fft=512, T=17, R=1, room_cov=1, frames=None, chunks=0, store_z=True, solve='auto', **_):
    """disco_selftest_staged_step2 on an exact scene: route, z, every pencil's matrices, their leading block against
    disco_cov_masked(P = M), and -- where every room holds >= 4 P frames -- the pending solve under both loaders.  store_z = False (room
    pass): the sums identical to the storing run's, z untouched."""
    F = n_fft // 2 + 1
    P = M + K - 1
    fr = np.full(R, T) if frames is None else np.asarray(frames)
    assert fr.shape == (R,) and fr.max() == T
    want = expected_route(M, K, room_cov)
    what = f'{kernel_of(M, K, n_fft, room_cov)} (M={M} K={K} n_fft={n_fft} T={T} R={R} frames={frames} chunks={chunks} store_z={store_z})'
    solvable = (solve == 'auto' and fr.min() >= 4 * P) or solve is True
    out = {}
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if frames is not None else None)
    try:
        eng.set_option('room_cov', room_cov)
        if chunks:
            eng.set_tuning(cov_chunks=chunks)
        if frames is not None:
            eng.set_lengths(_lengths_of(fr, n_fft))
            assert np.array_equal(eng.frames, fr)
        for solv in ((False, True) if solvable else (False,)):
            X, _zs, _zn, mask = cc.scene(_seed(M, K, n_fft, T, R, 23 + solv), R, K, M, T, F, False, solvable=solv)
            if not solv:                                                  # whole bins of mask 0 and of mask 1
                assert (mask == 0).all(axis=2).any() and (mask == 1).all(axis=2).any()
            w_loc = room_filters(_seed(M, K, 29), R, K, F, M)
            garbage = np.random.default_rng(5).choice(np.array([-3.5, 0.0, 0.5, 1.0, 7.25], np.float32), mask.shape)
            for r in range(R):                                            # what the library's own spectra hold beyond a room's frames: zeros;
                X[r, :, fr[r]:] = 0                                       # a caller's mask: anything finite
                mask[r, :, fr[r]:] = garbage[r, :, fr[r]:]
            z_ref = exact_z(X, w_loc)
            zc = z_ref.astype(np.complex64)
            Sss, Snn = cc.ref_sums(X, mask, zc, zc, True, frames=fr)       # asserts the 2^24 bound: the z z^H terms are the largest
            _px, Xd = eng.to_device(X, np.complex64)
            _pm, md = eng.to_device(mask, np.float32)
            _pw, wd = eng.to_device(w_loc, np.complex64)
            zbuf = None if store_z else _pattern_z(eng, (R, K, T, F))
            z, route, Rss, Rnn = _run(eng, Xd, md, wd, P, store_z=store_z, z=zbuf, want_stages=ROUTE_STAGES[want])
            assert route == want, f'{what}: route {route}, expected {want}'
            if store_z or want != 'room':                                 # (disco_apply of the split route always writes z)
                bad = (z.astype(np.complex128) != z_ref).any(axis=2)
                assert not bad.any(), f'{what}: z differs from the exact w_loc^H X: {_first_bad(bad)}'
            else:
                assert (_bits(z) == Z_PATTERN).all(), f'{what}: store_z = 0 wrote to z'
            cc.compare_exact(Rss, Sss, fr, what + ' Rss')
            cc.compare_exact(Rnn, Snn, fr, what + ' Rnn')
            if not store_z and want == 'room':                            # the sums do not depend on whether z is stored
                _z2, _r2, Rss2, Rnn2 = _run(eng, Xd, md, wd, P, store_z=True)
                assert np.array_equal(_bits(Rss), _bits(Rss2)) and np.array_equal(_bits(Rnn), _bits(Rnn2)), f'{what}: store_z changes the sums'
                bad = (_z2.astype(np.complex128) != z_ref).any(axis=2)
                assert not bad.any(), f'{what}: z differs from the exact w_loc^H X: {_first_bad(bad)}'
            if solv:
                ref = cc.solve_bar(Sss / fr[:, None, None, None, None], Snn / fr[:, None, None, None, None], 1)
                for dpp in (0, 1):
                    eng.set_option('solve_dpp', dpp)
                    if dpp:
                        _run(eng, Xd, md, wd, P)                          # the pencil pending afresh
                    out[f'solve_dpp{dpp}'] = cc._check_solution(eng, P, ref, f'{what} solve_dpp={dpp}', min_floor_share=FLOOR_SHARE)
            # the leading M x M block is step 1's: bit-identical to the matrices disco_cov_masked(X, mask, P = M) hands out
            R1s, R1n = eng.cov_masked(Xd, md)
            for got, one, nm in ((Rss, R1s.numpy(), 'Rss'), (Rnn, R1n.numpy(), 'Rnn')):
                eq = _pencil_bits_equal(np.ascontiguousarray(got[..., :M, :M]), one)
                assert eq.all(), f'{what}: leading block of {nm} is not the step-1 matrix: {_first_bad(~eq)}'
    finally:
        eng.close()
    return out


def check_staged_cases(make_engine, cases):
    out = {}
    for c in cases:
        res = check_staged(make_engine, **c)
        if res:
            out[case_id(c)] = res
    return out


def check_nan_beyond(make_engine, M, K, n_fft=512, T=17, frames=(17, 1, 9), room_cov=1):
    """Every frame beyond a room's own T_r NaN in both X and mask: no output bit may change against the run with zeros there."""
    F = n_fft // 2 + 1
    P, R = M + K - 1, len(frames)
    fr = np.asarray(frames)
    what = f'{kernel_of(M, K, n_fft, room_cov)} (M={M} K={K} T={T} frames={frames})'
    X, _zs, _zn, mask = cc.scene(_seed(M, K, n_fft, T, R, 31), R, K, M, T, F, False)
    w_loc = room_filters(_seed(M, K, 29), R, K, F, M)
    Xn, mn = X.copy(), mask.copy()
    for r in range(R):
        X[r, :, fr[r]:] = 0
        Xn[r, :, fr[r]:] = np.nan
        mn[r, :, fr[r]:] = np.nan
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant')
    try:
        eng.set_option('room_cov', room_cov)
        eng.set_lengths(_lengths_of(fr, n_fft))
        clean = _run(eng, X, mask, w_loc, P)
        hit = _run(eng, Xn, mn, w_loc, P)
        assert clean[1] == hit[1] == expected_route(M, K, room_cov)
        for a, b, nm in ((clean[2], hit[2], 'Rss'), (clean[3], hit[3], 'Rnn')):
            eq = _pencil_bits_equal(a, b)
            n_nan = int(np.isnan(b).any(axis=(-1, -2)).sum())
            assert eq.all(), f'{what}: NaN beyond a room\'s frames moved {nm}: {_first_bad(~eq)} ({n_nan} pencils hold NaN)'
        neq = (_bits(clean[0]) != _bits(hit[0])).reshape(clean[0].shape + (2,)).any(axis=-1)
        assert not neq.any(), f'{what}: NaN beyond a room\'s frames moved z: {_first_bad(neq.any(axis=2))}'
    finally:
        eng.close()


def check_containment(make_engine, M, K, n_fft=512, T=17, R=2, room_cov=1):
    """One NaN in X at (r, k, t, f, m): only the pencils of bin f in room r may differ (every node of the room receives z_k); every other
    (room, bin) is bit-identical to the clean run, and so is every z but z[r, k, t, f]."""
    F = n_fft // 2 + 1
    P = M + K - 1
    r0, k0, t0, f0 = R - 1, min(1, K - 1), T // 2, 38
    what = f'{kernel_of(M, K, n_fft, room_cov)} (M={M} K={K} T={T} R={R})'
    X, _zs, _zn, mask = cc.scene(_seed(M, K, n_fft, T, R, 37), R, K, M, T, F, False)
    w_loc = room_filters(_seed(M, K, 29), R, K, F, M)
    Xn = X.copy()
    Xn[r0, k0, t0, f0, :] = np.nan                                        # whatever taps w_loc holds: z of node k0 is NaN there
    eng = _engine(make_engine, R, K, M, T, n_fft)
    try:
        eng.set_option('room_cov', room_cov)
        clean = _run(eng, X, mask, w_loc, P)
        hit = _run(eng, Xn, mask, w_loc, P)
        same = np.ones((R, K, F), bool)
        same[r0, :, f0] = False
        for a, b, nm in ((clean[2], hit[2], 'Rss'), (clean[3], hit[3], 'Rnn')):
            eq = _pencil_bits_equal(a, b)
            assert eq[same].all(), f'{what}: a NaN in X moved {nm} elsewhere: {_first_bad(~eq & same)}'
            assert np.isnan(b[r0, :, f0]).any(axis=(-1, -2)).all(), f'{what}: the NaN did not reach every pencil of its room and bin ({nm})'
        neq = (_bits(clean[0]) != _bits(hit[0])).reshape(clean[0].shape + (2,)).any(axis=-1)
        assert neq[r0, k0, t0, f0]
        neq[r0, k0, t0, f0] = False
        assert not neq.any(), f'{what}: z changed away from the NaN: {_first_bad(neq.any(axis=2))}'
    finally:
        eng.close()


# ---- the re-use route, exact ------------------------------------------------------------------------------------------------------------

def check_reuse_exact(make_engine, M, K, T=32, n_fft=512, R=1):
    """disco_cov_masked(X, mask, P = M, Rss = NULL) keeps the step-1 record of X / mask (api_cov.hip, step1_keep) and
    disco_step2_cov_fused_reuse grants the re-use for the same two arrays (api_step2_cov.hip: step1_any, step1_held): on an exact scene
    z_out, the matrices of the two-block pencil and its solve."""
    F = n_fft // 2 + 1
    P = M + K - 1
    what = f'k_step2_cov_fused<{M},{K},true> (n_fft={n_fft} T={T} R={R})'
    assert T >= 4 * P
    X, _zs, _zn, mask = cc.scene(_seed(M, K, n_fft, T, R, 41), R, K, M, T, F, False, solvable=True)
    w_loc = room_filters(_seed(M, K, 29), R, K, F, M)
    z_ref = exact_z(X, w_loc)
    zc = z_ref.astype(np.complex64)
    Sss, Snn = cc.ref_sums(X, mask, zc, zc, True)
    eng = _engine(make_engine, R, K, M, T, n_fft)
    try:
        _px, Xd = eng.to_device(X, np.complex64)                          # the re-use is granted for THE arrays step 1 saw
        _pm, md = eng.to_device(mask, np.float32)
        eng.cov_masked(Xd, md, Rss_out=False)
        z = eng.step2_cov_fused_reuse(Xd, md, w_loc, want_z=True).numpy()
        Rss, Rnn = eng.selftest_pending_matrices(P)
        bad = (z.astype(np.complex128) != z_ref).any(axis=2)
        assert not bad.any(), f'{what}: z_out differs from the exact z: {_first_bad(bad)}'
        fr = np.full(R, T)
        cc.compare_exact(Rss, Sss, fr, what + ' Rss')
        cc.compare_exact(Rnn, Snn, fr, what + ' Rnn')
        res = cc._check_solution(eng, P, cc.solve_bar(Sss, Snn, T), what, min_floor_share=FLOOR_SHARE)
        R1s, R1n = eng.cov_masked(Xd, md)
        for got, one, nm in ((Rss, R1s.numpy(), 'Rss'), (Rnn, R1n.numpy(), 'Rnn')):
            eq = _pencil_bits_equal(np.ascontiguousarray(got[..., :M, :M]), one)
            assert eq.all(), f'{what}: leading block of {nm} is not the step-1 matrix: {_first_bad(~eq)}'
    finally:
        eng.close()
    return res


# ---- the float tier ---------------------------------------------------------------------------------------------------------------------

FLOAT_SHAPES = ((8, 8), (4, 6))


def float_scene(M, K, T=cc.T_FLOAT, F=257):
    """X, mask of parity_checks._rand_stft_scene (one room) and random filters of unit expected norm: z carries the energy of a channel."""
    from parity_checks import _rand_stft_scene
    rng = np.random.default_rng(_seed(M, K, 43))
    X, mask = _rand_stft_scene(rng, 1, K, M, T, F)
    w = (rng.standard_normal((1, K, F, M)) + 1j * rng.standard_normal((1, K, F, M))) / np.sqrt(2.0 * M)
    return X, mask, w.astype(np.complex64)


def check_float(make_engine, M, K, room_cov, T=cc.T_FLOAT, n_fft=512):
    """-> {'fro', 'coh', 'bar_fro', 'bar_coh'}: worst per pencil against the float64 covariance of X and the float64 z = w_loc^H X; the
    bar is BAR_FACTOR x the worst distance of cov_f32_restatement of the same inputs (reference side, all T frames in one float32 run)."""
    F = n_fft // 2 + 1
    P = M + K - 1
    X, mask, w_loc = float_scene(M, K, T, F)
    z_ref = exact_z(X, w_loc)
    rs, rn = cc.float_ref(X, z_ref, mask, spread=1000.0)           # (a z row whose filter nearly misses the source is weak, not empty)
    a, b = cc.cov_f32_restatement(X, z_ref.astype(np.complex64), mask)
    qa, qb = cc.pencil_quantities(a, rs), cc.pencil_quantities(b, rn)
    dist = (float(max(qa[0].max(), qb[0].max())), float(max(qa[1].max(), qb[1].max())))
    what = f'{kernel_of(M, K, n_fft, room_cov)} T={T}'
    eng = _engine(make_engine, 1, K, M, T, n_fft)
    try:
        eng.set_option('room_cov', room_cov)
        eng.set_tuning(cov_chunks=1)
        z, route, Rss, Rnn = _run(eng, X, mask, w_loc, P)
        assert route == expected_route(M, K, room_cov), route
        scale = np.einsum('rkfm,rktfm->rktf', np.abs(w_loc.real).astype(np.float64) + np.abs(w_loc.imag),
                          np.abs(X.real).astype(np.float64) + np.abs(X.imag))
        bad = ~(np.abs(z - z_ref) <= 2 * M * 2.0 ** -24 * scale)          # 2 M products and sums per part, each rounded once
        assert not bad.any(), f'{what}: z is not w_loc^H X: {_first_bad(bad.any(axis=2))}'
        worst = [0.0, 0.0]
        for got, ref, nm in ((Rss, rs, 'Rss'), (Rnn, rn, 'Rnn')):
            for i, (q, qn) in enumerate(zip(cc.pencil_quantities(got, ref), ('fro', 'coh'))):
                bar = cc.BAR_FACTOR * dist[i]
                print('room_routes_float', what, nm, qn, f'worst {float(q.max()):.3e} bar {bar:.3e}')
                assert not (~(q <= bar)).any(), f'{what} {nm} {qn}: worst {float(q.max()):.3e}, bar {bar:.3e}: {_first_bad(~(q <= bar))}'
                worst[i] = max(worst[i], float(q.max()))
    finally:
        eng.close()
    return {'fro': worst[0], 'coh': worst[1], 'bar_fro': cc.BAR_FACTOR * dist[0], 'bar_coh': cc.BAR_FACTOR * dist[1]}
