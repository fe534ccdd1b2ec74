"""Checks of the filter-and-sum and inverse-transform kernels output by output (csrc/k_apply.h, csrc/k_fused.h k_step2_apply_fused /
k_step2_apply_istft / k_apply_istft_wide, csrc/k_stft.h k_istft), on every route of disco_apply, disco_step2_apply_fused,
disco_step2_apply_istft_fused, disco_apply_istft_fused and disco_istft, through Engine.apply / step2_apply_fused /
step2_apply_istft_fused / apply_istft / istft.

Shared by tests/test_gpu_apply_routes.py (real MI355X, `-m gpu`), tests/test_apply_routes_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut down) and tests/test_apply_routes_cpu.py (the reference side alone: the route table against the headers, the
coverage of the case lists, the restatement behind the inverse-transform bar).  `make_engine(**cfg)` builds a disco_amd.engine.Engine
bound to the library under test.

Route table (`route` below restates api_apply.hip / api_step2_apply.hip / api_step2_istft.hip / api_apply_istft_wide.hip / istft_any of
api_stft.hip; the CPU test reads the shape tables out of the headers and asserts that the case lists launch every name `route` returns):
    disco_apply (KR = P - M remote rows: 0 or K - 1)
        (M, KR) in DISCO_FOR_MKR (P <= 8)        k_apply<M, KR>                 flat over (t, f), 256 threads
        M = 4 | 8, 1 <= KR <= 15, not above      k_apply_mq<M, KRT>             KRT = 1 | 3 | 7 | 15 >= KR; rows KR .. KRT - 1 re-read row
                                                                                KR - 1 with a zero tap (KRT = 1 holds KR = 1 alone)
        KR >= 16 (17 <= P <= 32)                 k_apply_m<M, 31>               M = 1 .. 8
        anything else (M not 4 | 8, P <= M + 15) k_apply_m<M, 15>               M = 1, 2, 3, 5, 6, 7
    disco_step2_apply_fused                      k_step2_apply_fused<M, K>      every (M, K) with M + K - 1 <= 8; refused under a shard
    disco_step2_apply_istft_fused                k_step2_apply_istft<512, M, K> the same 36 shapes at 512 points, ApplyIstftShared within
                                                                                160 KiB (`apply_istft_shared_bytes`; all 36 fit)
    disco_apply_istft_fused                      k_apply_istft_wide<N, M, K-1>  N = 512 | 1024, the nine (M, K) of DISCO_FOR_WIDE_ISTFT
    disco_istft                                  k_istft<N, false>
    UNREACHABLE (instantiated, never launched): k_apply_mq<4, 1> and <4, 3> (KR <= 4 with four microphones is in DISCO_FOR_MKR, and disco_apply
        tries for_mkr first), k_apply_m<4, 15> and <8, 15> (every M = 4 | 8 call with 1 <= KR <= 15 runs k_apply or
        k_apply_mq, and KR = 0 is in the table).
    ELSEWHERE: k_istft<N, true> (one frame per transform) belongs to the online entry points (tests/online_checks.py);
        k_stft_apply_istft takes its filter from the solve inside disco_tango_enhance and cannot be given taps: whole-path tests only
        (tests/test_gpu_parity.py).

THE EXACT TIER.  A filter output is a sum of P complex products.  The scenes hold spectra (and caller-supplied z rows) whose real and
imaginary parts are integers in [-8, 8] and taps that are multiples of 1/4 in [-2, 2] (for the kernels that form z on chip: w_loc and
w_glo multiples of 1/2 in [-1, 1], so z is a multiple of 1/2 and yf of 1/4), with taps that are exactly 0 and whole bins of all-zero
filters, everything drawn independently per (room, node, bin).  Every product and every partial sum -- in any order, with or without
FMA contraction -- is then exactly representable in float32 as long as q x (the sum of the absolute values of an output's terms) stays
below 2^24, q the denominator of the grid the products live on (4; 16 with the inverse-transform tier's dither); `ref_apply` asserts
max(4, q) x that bound on the float64 reference of every case.  The kernels' outputs must then EQUAL the float64 einsum: every (room, node,
frame, bin) is compared on its own with ==; no entry is excluded.

THE INVERSE-TRANSFORM TIER.  The spectrum that enters the transform is known exactly (an exact scene, with a dither of +-1/4 on every
part of every spectrum entry so that no frame is quiet; asserted: the rms of every hop segment of the reference within a factor 2 of
its signal's).  Reference: oracle/stft_oracle.istft(..., work_dtype=float64) of the exact yf.  Quantity, per (room, node, hop
segment): max |out - ref| over the segment / rms(ref over the signal).  Bar, per (room, node, hop segment): BAR_FACTOR = 4 x the same
quantity of `istft_f32` -- scipy.fft.irfft on complex64, then window, overlap-add and window-sum division in float32 -- recomputed on
the reference side on the inputs of every run, never taken from a kernel's output.  The wave FFT (Stockham 8 x 8 x 8 / 16 x 16 x 4) and
pocketfft round in different places but in the same class; tests/cov_checks.py uses the same margin.  No segment is excluded; a
segment beyond a room's own length must be exactly 0 (its bar is 0).  Lengths keep L % hop <= hop / 2 (the project's rule for the
window-sum edge of the last segment).
"""
import numpy as np

from cov_checks import HOP, MKR, _bits, _engine, _raises, _seed, kernel_key, z_to_blocks
from oracle import stft_oracle as so

BAR_FACTOR = 4.0
ROOM = ((8, 8), (8, 6), (8, 4), (8, 2), (4, 8), (4, 6))                               # DISCO_FOR_ROOM (dispatch.h)
WIDE_ISTFT = ROOM + ((4, 4), (4, 3), (4, 2))                                          # DISCO_FOR_WIDE_ISTFT (dispatch.h)
MQ = tuple((m, krt) for m in (4, 8) for krt in (1, 3, 7, 15))                         # DISCO_FOR_APPLY_MQ (dispatch.h)
LDS_BUDGET = 160 * 1024
UNREACHABLE = ('k_apply_mq<4,1>', 'k_apply_mq<4,3>', 'k_apply_m<4,15>', 'k_apply_m<8,15>')
ELSEWHERE = {
    'k_istft<N,true>': 'the online entry points (tests/online_checks.py)',
    'k_stft_apply_istft<512,M>': 'disco_tango_enhance of a single node: the filter comes from the solve inside the call '
                                 '(tests/test_gpu_parity.py, whole path only)',
}
ENTRIES = ('apply', 'step2_fused', 'step2_istft', 'apply_istft', 'istft')


def apply_istft_shared_bytes(M, K, N=512):
    """sizeof(ApplyIstftShared<N, M, K>) (k_fused.h): buf[K][fft_buf_len<N>()], zbuf[2][K][ZF], wl[K][ZF][M] of c32, ZF = N / 2 + 1 for
    K > 1 else 1, rounded up to the struct's alignment of 16."""
    buf_len = N + (N >> (3 if N == 512 else 4))
    zf = N // 2 + 1 if K > 1 else 1
    return -(-(8 * (K * buf_len + 2 * K * zf + K * zf * M)) // 16) * 16


def krt_of(KR):
    return 1 if KR <= 1 else 3 if KR <= 3 else 7 if KR <= 7 else 15


def route(M, K, n_fft, entry, sharded=False, step2=True):
    """The kernel a call launches, as a tuple of one name; a refusal as ('refused: ...',).  entry: one of ENTRIES; step2 (disco_apply
    only): P = M + K - 1, else P = M."""
    assert n_fft in (512, 1024) and entry in ENTRIES
    if entry == 'istft':
        return (f'k_istft<{n_fft},false>',)
    if entry == 'apply':
        KR = K - 1 if step2 else 0
        if M > 8:
            return ('refused: more than 8 mics',)
        if M + KR > 32:
            return ('refused: P > 32',)
        if (M, KR) in MKR:
            return (f'k_apply<{M},{KR}>',)
        if M in (4, 8) and 1 <= KR <= 15:
            return (f'k_apply_mq<{M},{krt_of(KR)}>',)
        return (f'k_apply_m<{M},{31 if KR > 15 else 15}>',)
    if entry == 'apply_istft':
        if (M, K) not in WIDE_ISTFT:
            return ('refused: shape not built',)
        return (f'k_apply_istft_wide<{n_fft},{M},{K - 1}>',)
    if sharded:
        return ('refused: node shard',)
    if M + K - 1 > 8 or (M, K - 1) not in MKR:
        return ('refused: M + K - 1 > 8',)
    if entry == 'step2_fused':
        return (f'k_step2_apply_fused<{M},{K}>',)
    if n_fft != 512:
        return ('refused: needs n_fft = 512',)
    if apply_istft_shared_bytes(M, K) > LDS_BUDGET:
        return ('refused: LDS budget',)
    return (f'k_step2_apply_istft<512,{M},{K}>',)


def reachable():
    """Every kernel name `route` can return."""
    names = set()
    for n_fft in (512, 1024):
        for M in range(1, 10):
            for K in range(1, 35):
                for entry in ENTRIES:
                    names.update(route(M, K, n_fft, entry))
                names.update(route(M, K, n_fft, 'apply', step2=False))
    return {n for n in names if not n.startswith('refused')}


def instantiated():
    """Every instantiation the launches of the five files name (the shape tables of dispatch.h times their with_bool / for_int)."""
    inst = {f'k_apply<{m},{kr}>' for m, kr in MKR} | {f'k_apply_m<{m},{x}>' for m in range(1, 9) for x in (15, 31)}
    inst |= {f'k_apply_mq<{m},{krt}>' for m, krt in MQ} | {f'k_step2_apply_fused<{m},{kr + 1}>' for m, kr in MKR}
    inst |= {f'k_step2_apply_istft<512,{m},{kr + 1}>' for m, kr in MKR if apply_istft_shared_bytes(m, kr + 1) <= LDS_BUDGET}
    inst |= {f'k_apply_istft_wide<{n},{m},{k - 1}>' for n in (512, 1024) for m, k in WIDE_ISTFT} | {'k_istft<512,false>', 'k_istft<1024,false>'}
    return inst


# ---- the lists of cases ---------------------------------------------------------------------------------------------------------------

T_DEFAULT = (1, 2, 3, 9)


def apply_cases(cut=False):
    """disco_apply: dicts (M, K, n_fft, step2, T).  Every k_apply<M, KR>; k_apply_m<M, 15> at its first, a middle and its last KR for
    every M that reaches it; k_apply_m<M, 31> at KR = 16 and at P = 32 for M = 1 .. 8; every reachable k_apply_mq<M, KRT> with KR < KRT
    (the zero-tap padding rows run) and KR = KRT; one case per family at 1024 points.  T walks T_DEFAULT.  cut: the emulator's list."""
    cases = []

    def add(M, K, n_fft=512, step2=True, T=None):
        c = dict(M=M, K=K, n_fft=n_fft, step2=step2, T=T_DEFAULT[len(cases) % 4] if T is None else T)
        if not any(all(c[k] == d[k] for k in ('M', 'K', 'n_fft', 'step2')) for d in cases):
            cases.append(c)
    if cut:
        for M in range(1, 9):                                            # every M of k_apply, with and without remote rows
            add(M, 2 if M % 2 else 1, step2=False, T=3)
            if M < 8:
                add(M, 9 - M if M % 2 else 2, T=3)
        for M in (1, 2, 3, 5, 6, 7):                                     # every M of k_apply_m<M, 15>
            add(M, 10 - M + (M % 3), T=3)
        for M in range(1, 9):                                            # every M of k_apply_m<M, 31>
            add(M, 17 + M % 2, T=2)
        for M, K in ((4, 6), (4, 8), (4, 10), (4, 16), (8, 2), (8, 3), (8, 4), (8, 6), (8, 8), (8, 10), (8, 16)):
            add(M, K, T=3)                                               # every reachable k_apply_mq, KR < KRT and KR = KRT
        add(2, 3, 1024, T=2)
        add(8, 4, 1024, T=2)
        add(3, 8, 1024, T=2)
        return cases
    for M, KR in MKR:
        if KR == 0:
            add(M, 1 if M % 2 else 3, step2=False)
        else:
            add(M, KR + 1)
    for M in (1, 2, 3, 5, 6, 7):
        for KR in (9 - M, 12, 15):
            add(M, KR + 1)
    for M in range(1, 9):
        add(M, 17)
        add(M, 33 - M)
    for M, KRs in ((4, (5, 6, 7, 8, 12, 15)), (8, (1, 2, 3, 4, 5, 7, 8, 11, 15))):
        for KR in KRs:
            add(M, KR + 1)
    for M, K in ((2, 3), (5, 1), (3, 8), (2, 18), (8, 4), (4, 7), (8, 10)):
        add(M, K, 1024, step2=K > 1)
    return cases


def fused_shapes():
    """Every (M, K) with M + K - 1 <= 8: the 36 shapes of k_step2_apply_fused and k_step2_apply_istft."""
    return [(M, KR + 1) for M, KR in MKR]


FUSED_CUT = [(M, min(9 - M, 3) if M < 8 else 1) for M in range(1, 9)] + [(1, 8), (4, 4), (2, 1)]
WIDE_CUT = [(512, 4, 2), (512, 8, 2), (1024, 4, 3), (512, 4, 8), (1024, 8, 4)]


def wide_shapes():
    return [(n, M, K) for n in (512, 1024) for M, K in WIDE_ISTFT]


def launched_by_exact(cut=False):
    """Names launched by the exact tier's lists."""
    names = set()
    for c in apply_cases(cut):
        names.update(route(c['M'], c['K'], c['n_fft'], 'apply', step2=c['step2']))
    for M, K in (FUSED_CUT if cut else fused_shapes()):
        names.update(route(M, K, 512, 'step2_fused'))
    for n, M, K in (WIDE_CUT if cut else wide_shapes()):
        names.update(route(M, K, n, 'apply_istft'))
    return names


def launched_by_istft(cut=False):
    names = set()
    for c in istft_cases(cut):
        names.update(route(c['M'], c['K'], c['n_fft'], c['entry']))
    return names


# ---- scenes whose filter outputs are exact ----------------------------------------------------------------------------------------------

def _cgrid(rng, lim, step, shape):
    n = int(round(lim / step))
    return ((rng.integers(-n, n + 1, shape) + 1j * rng.integers(-n, n + 1, shape)) * step).astype(np.complex64)


def spectra(rng, shape, dither=False):
    """Integer parts in [-8, 8]; dither: +-1/4 on every part (no quiet frame; the products move to the 1/16 grid)."""
    x = _cgrid(rng, 8, 1, shape)
    if dither:
        x = x + ((2 * rng.integers(0, 2, shape) - 1) + 1j * (2 * rng.integers(0, 2, shape) - 1)).astype(np.complex64) * np.float32(0.25)
    return x.astype(np.complex64)


def taps(rng, R, K, F, P, step, lim):
    """(R, K, F, P) multiples of `step` in [-lim, lim]; one tap in five exactly 0; whole bins of all-zero filters."""
    w = _cgrid(rng, lim, step, (R, K, F, P))
    w[rng.integers(0, 5, w.shape) == 0] = 0
    sel = (np.arange(F)[None, None, :] + np.arange(R)[:, None, None] + 3 * np.arange(K)[None, :, None]) % 7
    w[sel == 3] = 0
    return w


def rows_all(X, Z, nodes):
    """(R, Kl, T, F, P) complex128: [X_k ; z_j, j < k ; z_j, j > k] of the global nodes `nodes` (X holds those, Z all K)."""
    X = X.astype(np.complex128)
    if Z is None:
        return X
    K = Z.shape[1]
    out = []
    for kl, k in enumerate(nodes):
        others = [j for j in range(K) if j != k]
        zr = np.moveaxis(Z[:, others].astype(np.complex128), 1, -1)
        out.append(np.concatenate([X[:, kl], zr], axis=-1))
    return np.stack(out, axis=1)


def ref_apply(X, Z, w, conj=True, nodes=None, q=4):
    """float64 restatement of tango.py:369-374 / 445-450: out[r, k, t, f] = sum_p c(w[r, k, f, p]) v[r, k, t, f, p].  Asserts the
    headroom of the exact tier: 4 x sum |terms| < 2^24 for every output, and that the result lives on the 1 / q grid."""
    nodes = list(range(X.shape[1])) if nodes is None else list(nodes)
    V = rows_all(X, Z, nodes)
    W = w.astype(np.complex128)
    assert W.shape[-1] == V.shape[-1], (W.shape, V.shape)
    out = np.einsum('rkfp,rktfp->rktf', W.conj() if conj else W, V)
    bound = np.einsum('rkfp,rktfp->rktf', np.abs(W.real) + np.abs(W.imag), np.abs(V.real) + np.abs(V.imag))
    worst = float(bound.max()) if bound.size else 0.0
    assert max(4, q) * worst < 2.0 ** 24, f'test bug: the scene breaks the representability bound ({max(4, q)} x {worst:.3g} >= 2^24)'
    assert np.array_equal(out * q, np.round(out.real * q) + 1j * np.round(out.imag * q))     # on the 1 / q grid: the float64 sums are the exact sums
    return out


def compare_bits(got, ref, what):
    """got complex64 from the library, ref the exact float64 values: every (room, node, frame, bin) must be equal."""
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = ~((got.real.astype(np.float64) == ref.real) & (got.imag.astype(np.float64) == ref.imag))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} outputs differ from the exact sums; first (room, node, frame, bin) {i}: '
                             f'got {complex(got[i])}, exact {complex(ref[i])}')


def same_bits(a, b):
    """complex64 / float32 arrays -> bool array: bit-identical entries."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == np.complex64:
        return (_bits(a).reshape(a.shape + (2,)) == _bits(b).reshape(b.shape + (2,))).all(axis=-1)
    return _bits(a) == _bits(b)


def apply_scene(seed, R, K, M, T, F, step2=True, dither=False):
    rng = np.random.default_rng(seed)
    X = spectra(rng, (R, K, T, F, M), dither)
    Z = spectra(rng, (R, K, T, F), dither) if step2 and K > 1 else None
    w = taps(rng, R, K, F, M + (K - 1 if Z is not None else 0), 0.25, 2)
    return X, Z, w


def onchip_scene(seed, R, K, M, T, F, dither=False):
    rng = np.random.default_rng(seed)
    X = spectra(rng, (R, K, T, F, M), dither)
    return X, taps(rng, R, K, F, M, 0.5, 1), taps(rng, R, K, F, M + K - 1, 0.5, 1)


def ref_onchip(X, w_loc, w_glo, q=4):
    """-> z, yf (float64, exact): z = w_loc^H X, yf = w_glo^H [X ; z_-k]."""
    K = X.shape[1]
    z = ref_apply(X, None, w_loc, q=q)
    zc = z.astype(np.complex64)
    assert np.array_equal(zc.astype(np.complex128), z)
    return z, ref_apply(X, zc if K > 1 else None, w_glo, q=q)


def check_apply(make_engine, M, K, n_fft=512, step2=True, T=3, R=2, conjs=(True, False), shard=None, zblk=None, lengths_frames=None, **_):
    """disco_apply on an exact scene: every output against the exact sums, for conj_w = 1 and 0.  -> {conj: out}."""
    F = n_fft // 2 + 1
    X, Z, w = apply_scene(_seed(M, K, n_fft, step2, T, R), R, K, M, T, F, step2)
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if lengths_frames is not None else None)
    outs = {}
    try:
        if lengths_frames is not None:
            eng.set_lengths([(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in lengths_frames])
            assert np.array_equal(eng.frames, lengths_frames)
            for r in range(R):
                X[r, :, lengths_frames[r]:] = 0
                if Z is not None:
                    Z[r, :, lengths_frames[r]:] = 0
        nodes, Xl, wl = list(range(K)), X, w
        if shard is not None:
            k0, Kl = shard
            eng.set_node_shard(k0, Kl)
            nodes = list(range(k0, k0 + Kl))
            Xl, wl = np.ascontiguousarray(X[:, nodes]), np.ascontiguousarray(w[:, nodes])
        z_in = Z
        if zblk is not None and Z is not None:
            eng.set_z_blocks(zblk)
            z_in = z_to_blocks(Z, zblk)
        name = route(M, K, n_fft, 'apply', step2=step2)[0]
        for conj in conjs:
            got = eng.apply(Xl, wl, Z=z_in, conj=conj).numpy()
            what = f'{name} (M={M} K={K} n_fft={n_fft} T={T} R={R} conj_w={int(conj)} shard={shard} zblk={zblk} frames={lengths_frames})'
            compare_bits(got, ref_apply(Xl, Z, wl, conj, nodes), what)
            if lengths_frames is not None:
                for r in range(R):
                    assert not _bits(got[r, :, lengths_frames[r]:]).any(), f'{what}: room {r} is not exactly 0 beyond its frames'
            outs[conj] = got
    finally:
        eng.close()
    return outs


def check_apply_cases(make_engine, cases, **over):
    names = set()
    for c in cases:
        check_apply(make_engine, **dict(c, **over))
        names.update(route(c['M'], c['K'], c['n_fft'], 'apply', step2=c['step2']))
    return sorted(names)


def check_step2_fused(make_engine, M, K, n_fft=512, T=3, R=2, chunks=0, lengths_frames=None):
    """disco_step2_apply_fused on an exact scene: yf and z_out against the exact values, and the run without z_out bit-identical."""
    F = n_fft // 2 + 1
    X, w_loc, w_glo = onchip_scene(_seed(M, K, n_fft, T, R, 21), R, K, M, T, F)
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if lengths_frames is not None else None)
    try:
        if chunks:
            eng.set_tuning(step2_chunks=chunks)
        if lengths_frames is not None:
            eng.set_lengths([(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in lengths_frames])
            for r in range(R):
                X[r, :, lengths_frames[r]:] = 0
        z_ref, yf_ref = ref_onchip(X, w_loc, w_glo)
        yf, z = eng.step2_apply_fused(X, w_loc, w_glo, want_z=True)
        yf, z = yf.numpy(), z.numpy()
        what = f'k_step2_apply_fused<{M},{K}> (n_fft={n_fft} T={T} R={R} chunks={chunks} frames={lengths_frames})'
        compare_bits(z, z_ref, what + ' z_out')
        compare_bits(yf, yf_ref, what + ' yf')
        yf2, _none = eng.step2_apply_fused(X, w_loc, w_glo, want_z=False)
        assert same_bits(yf2.numpy(), yf).all(), what + ': yf depends on z_out being asked for'
    finally:
        eng.close()
    return yf


def check_wide_yf(make_engine, n_fft, M, K, T=3, R=2, shard=None, zblk=None, pairs=0, lengths_frames=None):
    """disco_apply_istft_fused with a yf buffer on an exact scene: the filtered spectra against the exact sums (the samples are the
    inverse-transform tier's business)."""
    F = n_fft // 2 + 1
    X, Z, w = apply_scene(_seed(M, K, n_fft, T, R, 31), R, K, M, T, F)
    eng = _engine(make_engine, R, K, M, T, n_fft, 'constant' if lengths_frames is not None else None)
    try:
        if pairs:
            eng.set_tuning(istft_pairs=pairs)
        if lengths_frames is not None:
            eng.set_lengths([(int(t) - 1) * HOP[n_fft] + (1 if t == 1 else 0) for t in lengths_frames])
            for r in range(R):
                X[r, :, lengths_frames[r]:] = 0
                Z[r, :, lengths_frames[r]:] = 0
        nodes, Xl, wl = list(range(K)), X, w
        if shard is not None:
            k0, Kl = shard
            eng.set_node_shard(k0, Kl)
            nodes = list(range(k0, k0 + Kl))
            Xl, wl = np.ascontiguousarray(X[:, nodes]), np.ascontiguousarray(w[:, nodes])
        z_in = Z
        if zblk is not None:
            eng.set_z_blocks(zblk)
            z_in = z_to_blocks(Z, zblk)
        buf = eng.empty((R, len(nodes), T, F), np.complex64)
        out = eng.apply_istft(Xl, wl, z_in, yf_out=buf)
        what = f'k_apply_istft_wide<{n_fft},{M},{K - 1}> (T={T} R={R} shard={shard} zblk={zblk} pairs={pairs} frames={lengths_frames}) yf'
        assert out is not None, what + ': refused'
        got = buf.numpy()
        compare_bits(got, ref_apply(Xl, Z, wl, True, nodes), what)
        assert np.isfinite(out.numpy()).all(), what + ': non-finite samples'
    finally:
        eng.close()
    return got


def check_heads_and_residuals(make_engine, shapes=((2, 3, 0), (8, 2, 5))):
    """disco_filter_head and disco_noise_residual: copies and one subtraction of integers -- bit-exact.  shapes: (M, K, ref_mic)."""
    for M, K, ref in shapes:
        T, F, R = 3, 257, 2
        X, Z, w = apply_scene(_seed(M, K, ref, 41), R, K, M, T, F)
        eng = make_engine(rooms=R, nodes=K, mics=M, length=(T - 1) * 256, n_fft=512, ref_mic=ref)
        try:
            head = eng.filter_head(w).numpy()
            assert head.shape == (R, K, F, M) and same_bits(head, np.ascontiguousarray(w[..., :M])).all(), f'disco_filter_head M={M} K={K}'
            zn = eng.noise_residual(X, Z).numpy()
            compare_bits(zn, X[..., ref].astype(np.complex128) - Z.astype(np.complex128), f'disco_noise_residual M={M} K={K} ref={ref}')
            eng.set_node_shard(K - 1, 1)                                  # the head honours the shard: the shard's nodes in, the same out
            head = eng.filter_head(np.ascontiguousarray(w[:, K - 1:])).numpy()
            assert same_bits(head, np.ascontiguousarray(w[:, K - 1:, :, :M])).all(), f'disco_filter_head under a shard M={M} K={K}'
        finally:
            eng.close()


# ---- launch geometry --------------------------------------------------------------------------------------------------------------------

# k_apply: T F below, at and above the 64-block cap of 256 threads (F = 257: 62 frames -> 63 blocks, 63 -> exactly 64, 64 and 128 ->
# capped, the loop strides); k_apply_m / k_apply_mq: one chunk (T < 16), T / 8 chunks of exactly 8 (16), ragged last chunks (17: 9 + 8;
# 25: 9 + 9 + 7) and a last chunk that is empty (81: ten chunks of 9, the tenth starts at 81)
GEOM_APPLY = {'k_apply': ((2, 3), (62, 63, 64, 128)), 'k_apply_m': ((3, 8), (9, 16, 17, 25, 81)), 'k_apply_m31': ((2, 18), (9, 16, 25, 81)),
              'k_apply_mq': ((8, 4), (9, 16, 17, 25, 81)), 'k_apply_mq4': ((4, 7), (16, 25, 81))}
# k_step2_apply_fused: (T, chunk count): 1, 2, 3 chunks, a count above T, and 1, 63, 64, 65, 129 frames for the Nyquist workgroup
GEOM_FUSED = ((1, 0), (1, 3), (2, 700), (3, 2), (63, 1), (64, 1), (64, 3), (65, 1), (65, 2), (129, 1), (129, 3), (130, 2), (9, 0))


def check_geometry_apply(make_engine, families=None, geom=GEOM_APPLY):
    done = []
    for fam, ((M, K), Ts) in geom.items():
        if families is not None and fam not in families:
            continue
        for T in Ts:
            check_apply(make_engine, M, K, 512, True, T=T)
            done.append((fam, T))
    return done


def check_geometry_fused(make_engine, geom=GEOM_FUSED, shapes=((2, 3), (4, 4))):
    done = []
    for i, (T, chunks) in enumerate(geom):
        M, K = shapes[i % len(shapes)]
        check_step2_fused(make_engine, M, K, 512, T=T, chunks=chunks)
        done.append((M, K, T, chunks))
    return done


# ---- node shards, z blocks, lengths ------------------------------------------------------------------------------------------------------

def check_shards(make_engine, T=3, every_k0=True, wide=True):
    """set_node_shard at every k0 of K = 4 through k_apply (M = 4), k_apply_m (M = 6), k_apply_mq (M = 8) and k_apply_istft_wide (M = 4),
    pairs of nodes with rank-major z blocks, three k0 of an 18-node network (k_apply_m<2, 31>, k_apply_m<4, 31>): the exact sums, and
    the same nodes of the unsharded run to the bit."""
    done = []
    for M, K in ((4, 4), (6, 4), (8, 4)):
        full = check_apply(make_engine, M, K, T=T)
        for k0 in (range(K) if every_k0 else (0, K - 1)):
            part = check_apply(make_engine, M, K, T=T, shard=(k0, 1), zblk=(2 if k0 % 2 else None))
            for c in full:
                assert same_bits(part[c], full[c][:, k0:k0 + 1]).all(), (M, K, k0, c)
            done.append((M, K, k0, 1))
        for k0 in (0, 2):
            part = check_apply(make_engine, M, K, T=T, shard=(k0, 2), zblk=2)
            for c in full:
                assert same_bits(part[c], full[c][:, k0:k0 + 2]).all(), (M, K, k0, c)
            done.append((M, K, k0, 2))
        check_apply(make_engine, M, K, T=T, zblk=1)
    full = check_wide_yf(make_engine, 512, 4, 4, T=T)
    for k0 in (range(4) if every_k0 else (1, 3)):
        part = check_wide_yf(make_engine, 512, 4, 4, T=T, shard=(k0, 1), zblk=(1 if k0 % 2 else None))
        assert same_bits(part, full[:, k0:k0 + 1]).all(), ('wide', k0)
        done.append(('wide', 4, 4, k0, 1))
    part = check_wide_yf(make_engine, 512, 4, 4, T=T, shard=(2, 2), zblk=2)
    assert same_bits(part, full[:, 2:4]).all()
    if wide:
        for M in (2, 4):
            full = check_apply(make_engine, M, 18, T=T, conjs=(True,))
            for k0 in (0, 9, 17):
                part = check_apply(make_engine, M, 18, T=T, conjs=(True,), shard=(k0, 1), zblk=3 if k0 else None)
                assert same_bits(part[True], full[True][:, k0:k0 + 1]).all(), (M, 18, k0)
                done.append((M, 18, k0, 1))
    return done


def check_lengths(make_engine, T=25):
    """Per-room lengths on the filter outputs: a room that ends inside a chunk (frame runs of 9 at T = 25: T_r = 13), a one-frame room,
    a full room.  Frames below T_r exact, frames beyond exact zeros (X and Z hold zeros there)."""
    frames = [13, 1, T] if T >= 16 else [T - 1, 1, T]
    for M, K in ((2, 3), (3, 8), (8, 4), (2, 18)):
        check_apply(make_engine, M, K, T=T, R=3, lengths_frames=frames)
    check_step2_fused(make_engine, 2, 3, T=T, R=3, chunks=2, lengths_frames=frames)
    check_step2_fused(make_engine, 4, 4, T=T, R=3, chunks=3, lengths_frames=frames[::-1])
    check_wide_yf(make_engine, 512, 4, 3, T=T, R=3, pairs=2, lengths_frames=frames)
    check_wide_yf(make_engine, 1024, 8, 2, T=T, R=3, pairs=3, lengths_frames=frames[::-1])
    return frames


# ---- a non-finite input stays where it is ---------------------------------------------------------------------------------------------

def check_nonfinite(make_engine, T=9, shapes=((2, 3), (3, 8), (4, 6), (8, 4), (2, 18))):
    """One NaN in X, or in a z row, at one (room, node, frame, bin): the outputs it reaches by the algebra -- its own node's at that
    (frame, bin) for X, every OTHER node's of that room for a z row, a zero tap included (0 x NaN) -- are non-finite, every other output
    is bit-identical to the clean run.  The z row is the LAST remote row of every node before it, which in the k_apply_mq<4, 7> case
    (K = 6: KR = 5 < KRT) is the row the zero-tap padding re-reads."""
    R, F = 2, 257
    r0, t0, f0 = 1, T // 2, 193
    for M, K in shapes:
        X, Z, w = apply_scene(_seed(M, K, 51), R, K, M, T, F)
        name = route(M, K, 512, 'apply')[0]
        eng = _engine(make_engine, R, K, M, T, 512)
        try:
            clean = eng.apply(X, w, Z=Z).numpy()
            Xn = X.copy()
            Xn[r0, 1, t0, f0, M - 1] = np.nan
            hit = eng.apply(Xn, w, Z=Z).numpy()
            reach = np.zeros(clean.shape, bool)
            reach[r0, 1, t0, f0] = True
            assert same_bits(clean, hit)[~reach].all(), f'{name}: a NaN in X moved {int((~same_bits(clean, hit) & ~reach).sum())} other outputs'
            assert not np.isfinite(hit[reach]).any(), f'{name}: the NaN in X did not reach its own output'
            Zn = Z.copy()
            Zn[r0, K - 1, t0, f0] = np.nan
            hit = eng.apply(X, w, Z=Zn).numpy()
            reach = np.zeros(clean.shape, bool)
            reach[r0, :K - 1, t0, f0] = True
            assert same_bits(clean, hit)[~reach].all(), f'{name}: a NaN in a z row moved {int((~same_bits(clean, hit) & ~reach).sum())} other outputs'
            assert not np.isfinite(hit[reach].real + hit[reach].imag).any(), f'{name}: the NaN in the z row did not reach every other node'
        finally:
            eng.close()
    M, K = 2, 3
    X, w_loc, w_glo = onchip_scene(_seed(M, K, 52), R, K, M, T, F)
    eng = _engine(make_engine, R, K, M, T, 512)
    try:
        eng.set_tuning(step2_chunks=2)
        yc, zc = (a.numpy() for a in eng.step2_apply_fused(X, w_loc, w_glo, want_z=True))
        Xn = X.copy()
        Xn[r0, 1, t0, f0, :] = np.nan
        yh, zh = (a.numpy() for a in eng.step2_apply_fused(Xn, w_loc, w_glo, want_z=True))
        reach = np.zeros(yc.shape, bool)
        reach[r0, :, t0, f0] = True                                      # every node of the room receives it through z
        assert same_bits(yc, yh)[~reach].all() and not np.isfinite(yh[reach].real + yh[reach].imag).any(), 'k_step2_apply_fused: yf'
        reach[:] = False
        reach[r0, 1, t0, f0] = True
        assert same_bits(zc, zh)[~reach].all() and not np.isfinite(zh[reach]).any(), 'k_step2_apply_fused: z_out'
    finally:
        eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def check_refusals(make_engine):
    """Each refusal returns its documented code (-1 DISCO_E_ARG, -2 DISCO_E_UNSUPPORTED) and leaves the context usable."""
    T, F = 2, 257

    def dev(eng, a):
        return eng.to_device(a, np.complex64)

    def err(eng):
        return eng.lib.disco_last_error(eng.ctx).decode()

    def usable(eng, X, Z, w):
        compare_bits(eng.apply(X, w, Z=Z).numpy(), ref_apply(X, Z, w), 'after a refusal')

    X, Z, w = apply_scene(1, 1, 3, 2, T, F)
    X_, wl_, wg_ = onchip_scene(2, 1, 3, 2, T, F)
    eng = _engine(make_engine, 1, 3, 2, T, 512)
    try:
        (px, _a), (pz, _b), (pw, _c), (pl, _d), (pg, _e) = dev(eng, X), dev(eng, Z), dev(eng, w), dev(eng, wl_), dev(eng, wg_)
        out = eng.empty((3 * T * F,), np.complex64)
        sig = eng.empty((3 * eng.Lsamp + 8,), np.float32)
        lib, ctx, s = eng.lib, eng.ctx, eng.stream
        for args in ((None, pz, pw, 4, 1, out.ptr), (px, pz, None, 4, 1, out.ptr), (px, pz, pw, 4, 1, None)):
            assert lib.disco_apply(ctx, *args, s) == -1 and 'null argument' in err(eng), err(eng)
        assert lib.disco_apply(ctx, px, pz, pw, 3, 1, out.ptr, s) == -1 and 'P must be M or M + K - 1' in err(eng), err(eng)
        assert lib.disco_apply(ctx, px, None, pw, 4, 1, out.ptr, s) == -1 and 'Z required' in err(eng), err(eng)
        for args in ((None, pl, pg, None, out.ptr), (px, None, pg, None, out.ptr), (px, pl, None, None, out.ptr), (px, pl, pg, None, None)):
            assert lib.disco_step2_apply_fused(ctx, *args, s) == -1 and 'null argument' in err(eng), err(eng)
        assert lib.disco_step2_apply_istft_fused(ctx, px, pl, pg, None, s) == -1 and 'null argument' in err(eng), err(eng)
        assert lib.disco_apply_istft_fused(ctx, px, None, pw, None, sig.ptr, s) == -1 and 'null argument' in err(eng), err(eng)
        assert lib.disco_apply_istft_fused(ctx, px, pz, pw, None, sig.ptr, s) == -2 and 'shape not built' in err(eng), err(eng)
        assert lib.disco_filter_head(ctx, None, 4, out.ptr, s) == -1 and lib.disco_filter_head(ctx, pw, 1, out.ptr, s) == -1 and 'P < M' in err(eng)
        assert lib.disco_noise_residual(ctx, px, None, out.ptr, s) == -1 and 'null argument' in err(eng), err(eng)
        assert lib.disco_istft(ctx, None, 3, sig.ptr, s) == -1 and lib.disco_istft(ctx, out.ptr, 0, sig.ptr, s) == -1, err(eng)
        usable(eng, X, Z, w)
        eng.set_node_shard(1, 1)                                         # the kernels that keep z on chip need the whole room
        assert lib.disco_step2_apply_fused(ctx, px, pl, pg, None, out.ptr, s) == -2 and 'node shard' in err(eng), err(eng)
        assert lib.disco_step2_apply_istft_fused(ctx, px, pl, pg, sig.ptr, s) == -2 and 'node shard' in err(eng), err(eng)
        eng.set_node_shard(0, 3)
        usable(eng, X, Z, w)
        compare_bits(eng.step2_apply_fused(X_, wl_, wg_)[0].numpy(), ref_onchip(X_, wl_, wg_)[1], 'after a refusal')
    finally:
        eng.close()
    for M, K, P, want in ((9, 1, 9, 'more than 8 mics'), (8, 26, 33, 'P = M + K - 1 > 32')):
        eng = _engine(make_engine, 1, K, M, T, 512)
        try:
            zeros = np.zeros((1, K, T, F, max(M, P)), np.complex64)
            (px, _a), out = dev(eng, zeros), eng.empty((K * T * F,), np.complex64)
            assert eng.lib.disco_apply(eng.ctx, px, px, px, P, 1, out.ptr, eng.stream) == -2 and want in err(eng), err(eng)
        finally:
            eng.close()
    X, Z, w = apply_scene(3, 1, 5, 5, T, F)                              # P = 9: the on-chip kernels refuse, disco_apply runs k_apply_m
    X_, wl_, wg_ = onchip_scene(4, 1, 5, 5, T, F)
    eng = _engine(make_engine, 1, 5, 5, T, 512)
    try:
        with _raises(eng, -2, 'M + K - 1 > 8'):
            eng.step2_apply_fused(X_, wl_, wg_)
        with _raises(eng, -2, 'M + K - 1 <= 8'):
            eng.step2_apply_istft_fused(X_, wl_, wg_)
        usable(eng, X, Z, w)
    finally:
        eng.close()
    X_, wl_, wg_ = onchip_scene(5, 1, 2, 2, T, 513)                      # 1024 points: the filter + transform kernel refuses, the filter runs
    eng = _engine(make_engine, 1, 2, 2, T, 1024)
    try:
        with _raises(eng, -2, 'needs n_fft = 512'):
            eng.step2_apply_istft_fused(X_, wl_, wg_)
        compare_bits(eng.step2_apply_fused(X_, wl_, wg_)[0].numpy(), ref_onchip(X_, wl_, wg_)[1], 'after a refusal')
    finally:
        eng.close()


# ---- more than 2^31 elements in X: the 64-bit offsets -----------------------------------------------------------------------------------

HUGE = {'k_apply': (4, 4, 840), 'k_apply_mq': (8, 2, 840)}              # family: (M, K, rooms): rooms x K x 626 x 257 x M > 2^31


def check_huge(make_engine, device, rooms=None, T=626):
    """X beyond 2^31 complex elements (17 GB), generated on the device with torch as exact inputs; the first and the last room are
    brought to the host and compared exactly, every node, frame and bin: a 32-bit offset anywhere lands the last room on other data."""
    import torch
    out = {}
    for name, (M, K, R) in HUGE.items():
        R = R if rooms is None else rooms
        F, P = 257, M + K - 1
        if rooms is None:
            assert R * K * T * F * M > 2 ** 31
        assert route(M, K, 512, 'apply')[0].startswith(name + '<')
        g = torch.Generator(device=device)
        g.manual_seed(_seed(M, K, 17))

        def grid(lim, step, *shape):
            n = int(round(lim / step))
            return torch.view_as_complex(torch.randint(-n, n + 1, shape + (2,), device=device, generator=g, dtype=torch.int8).to(torch.float32) * step)
        X, Z, w = grid(8, 1, R, K, T, F, M), grid(8, 1, R, K, T, F), grid(2, 0.25, R, K, F, P)
        if device != 'cpu':
            torch.cuda.synchronize()
        eng = _engine(make_engine, R, K, M, T, 512)
        try:
            got = eng.apply(X, w, Z=Z)
            ends = [0, R - 1]
            ref = ref_apply(X[ends].cpu().numpy(), Z[ends].cpu().numpy(), w[ends].cpu().numpy())
            per = T * F * K * 8                                           # bytes of one room of the output: only the two rooms travel
            host = np.empty((2, K, T, F), np.complex64)
            for i, r in enumerate(ends):
                eng._chk(eng.lib.disco_d2h(eng.ctx, host[i].ctypes.data, got.ptr + r * per, per, None))
            eng.sync()
            compare_bits(host, ref, f'{route(M, K, 512, "apply")[0]} with {R * K * T * F * M} elements in X, rooms 0 and {R - 1}')
            out[name] = R * K * T * F * M
        finally:
            eng.close()
        del X, Z, w, got
    return out


# ---- the inverse-transform tier -----------------------------------------------------------------------------------------------------------

def istft_f64(Y, L, n_fft):
    """Y (..., T, F) -> (..., L) float64: the oracle."""
    return so.istft(np.swapaxes(np.asarray(Y), -1, -2), L, n_fft, n_fft // 2, work_dtype=np.float64)


def istft_f32(Y, L, n_fft):
    """The float32 restatement behind the bar: scipy.fft.irfft on complex64 (single-precision pocketfft), then window, overlap-add and
    window-sum division in float32.  Y (..., T, F) -> (..., L) float32."""
    import scipy.fft
    Y = np.asarray(Y).astype(np.complex64)
    hop, T = n_fft // 2, Y.shape[-2]
    fr = scipy.fft.irfft(Y, n=n_fft, axis=-1)
    assert fr.dtype == np.float32
    fr = fr * so.hann_periodic(n_fft).astype(np.float32)
    n = n_fft + hop * (T - 1)
    y = np.zeros(Y.shape[:-2] + (n,), np.float32)
    for t in range(T):
        y[..., t * hop:t * hop + n_fft] += fr[..., t, :]
    env = so.window_sumsquare(T, n_fft, hop, dtype=np.float32)
    nz = env > np.finfo(np.float32).tiny
    y[..., nz] /= env[nz]
    y = y[..., n_fft // 2:]
    if y.shape[-1] < L:
        y = np.concatenate([y, np.zeros(y.shape[:-1] + (L - y.shape[-1],), np.float32)], axis=-1)
    assert y.dtype == np.float32
    return y[..., :L]


def room_wise(fn, Y, L, n_fft, lengths):
    """fn(Y, L, n_fft) with every room processed as if run alone at its own length (disco_set_lengths); zeros beyond."""
    if lengths is None:
        return fn(Y, L, n_fft)
    out = np.zeros(Y.shape[:-2] + (L,), np.float64 if fn is istft_f64 else np.float32)
    for r, Lr in enumerate(lengths):
        out[r, ..., :Lr] = fn(Y[r][..., :1 + Lr // (n_fft // 2), :], int(Lr), n_fft)
    return out


def segment_quantity(out, ref, hop, lengths=None, against=None):
    """(R, K, L) -> (R, K, n_seg): max |out - ref| over each hop segment / rms(ref over the room's own samples).  against: the
    distance is taken from this array instead (the staged calls' output), the normalisation stays the reference's."""
    R, K, L = ref.shape
    n_seg = -(-L // hop)
    d = np.zeros((R, K, n_seg * hop))
    d[..., :L] = np.abs(np.asarray(out, np.float64) - (ref if against is None else np.asarray(against, np.float64)))
    Ls = np.full(R, L) if lengths is None else np.asarray(lengths)
    rms = np.stack([np.sqrt(np.mean(ref[r, :, :Ls[r]] ** 2, axis=-1)) for r in range(R)])
    return d.reshape(R, K, n_seg, hop).max(-1) / rms[..., None]


def assert_segments_comparable(ref, hop, lengths=None):
    """The rms of every (live part of a) hop segment of the reference within a factor 2 of its signal's."""
    R, K, L = ref.shape
    for r in range(R):
        Lr = L if lengths is None else int(lengths[r])
        sig = np.sqrt(np.mean(ref[r, :, :Lr] ** 2, axis=-1))
        for s0 in range(0, Lr, hop):
            seg = np.sqrt(np.mean(ref[r, :, s0:min(s0 + hop, Lr)] ** 2, axis=-1))
            assert (seg < 2 * sig).all() and (seg > sig / 2).all(), f'test bug: segment {s0 // hop} of room {r}: rms {seg} against {sig}'


def length_of(n_seg, rem, hop):
    """A length with n_seg hop segments whose last holds `rem` samples (0: a whole one)."""
    assert 0 <= rem <= hop // 2
    return n_seg * hop if rem == 0 else (n_seg - 1) * hop + rem


def istft_cases(cut=False):
    """dicts (entry, M, K, n_fft, pairs, L[, lengths, staged]).  pairs: istft_pairs of set_tuning (0: the heuristic's choice, which for a
    small batch is 4 for k_step2_apply_istft and 2 for k_apply_istft_wide; k_istft has fixed blocks of 7 segments).  A run is
    2 pairs - 1 hop segments, a workgroup of k_apply_istft_wide holds n_fft / 256 runs.  Per kernel: n_seg exactly one run, one run
    plus one segment (the second run -- for the wide kernel the second workgroup, whose later runs are empty -- holds one), a multiple
    of the run; odd and even frame counts; L % hop zero and not; clips of 1, 2 and 3 frames; per-room lengths with a room ending inside
    a run, one ending before whole runs and a one-frame room; `staged`: also against the two staged calls on the same inputs.  A tail of
    a clip of several segments holds at least 64 samples, so that its rms is a statistic and not a draw (assert_segments_comparable)."""
    cases = []

    def add(entry, M, K, n_fft, pairs, n_seg, rem, lengths=None, staged=False):
        hop = n_fft // 2
        cases.append(dict(entry=entry, M=M, K=K, n_fft=n_fft, pairs=pairs, L=length_of(n_seg, rem, hop), staged=staged,
                          lengths=None if lengths is None else [length_of(a, b, hop) for a, b in lengths]))
    if cut:
        add('istft', 1, 2, 512, 0, 8, 100)
        add('istft', 1, 1, 1024, 0, 3, 0)
        add('step2_istft', 2, 2, 512, 2, 4, 124, staged=True)
        add('step2_istft', 1, 1, 512, 2, 2, 0)
        add('apply_istft', 4, 2, 512, 2, 7, 97, staged=True)
        add('apply_istft', 4, 2, 1024, 2, 4, 0)
        return cases
    for n_seg, rem in ((7, 0), (7, 100), (8, 0), (8, 128), (14, 65), (21, 0), (1, 77), (1, 0), (2, 100), (2, 0), (3, 114)):
        add('istft', 1, 2, 512, 0, n_seg, rem)                            # k_istft<512>: blocks of 7 segments; clips of 1, 2, 2, 3, 3 frames
    for n_seg, rem in ((7, 0), (8, 200), (15, 0), (2, 0)):
        add('istft', 1, 2, 1024, 0, n_seg, rem)
    add('istft', 1, 2, 512, 0, 20, 0, lengths=[(10, 100), (1, 17)])       # room 0 ends inside the second block, room 1 has one frame
    add('istft', 1, 3, 1024, 0, 16, 69, lengths=[(16, 69), (7, 0)])
    shapes = ((2, 2), (4, 4), (1, 1), (3, 2), (1, 8), (8, 1), (2, 5), (5, 4))
    i = 0
    for pairs in (2, 3, 4, 0, 64):                                        # k_step2_apply_istft<512, M, K>
        run = 2 * (pairs or 4) - 1
        for n_seg, rem in ((run, 0), (run, 90), (run + 1, 0), (run + 1, 128), (2 * run, 95), (3 * run if run < 100 else 2 * run, 0)):
            M, K = shapes[i % len(shapes)] if pairs != 64 else (2, 2)
            add('step2_istft', M, K, 512, pairs, n_seg, rem, staged=(i % 3 == 0))
            i += 1
    for n_seg, rem in ((1, 114), (1, 0), (2, 128), (2, 0), (3, 71)):        # clips of 1, 2, 2, 3, 3 frames
        add('step2_istft', 2, 3, 512, 2, n_seg, rem)
    for j, (M, K) in enumerate(fused_shapes()):                           # every instantiation, short clips
        add('step2_istft', M, K, 512, (2, 3, 0)[j % 3], 4 + j % 3, (0, 100)[j % 2])
    add('step2_istft', 2, 2, 512, 3, 17, 0, lengths=[(7, 104), (5, 0), (1, 100)])      # inside the second run; exactly one run; one frame
    add('step2_istft', 4, 4, 512, 2, 10, 100, lengths=[(10, 100), (2, 0), (1, 1)])
    i = 0
    for n_fft in (512, 1024):                                             # k_apply_istft_wide<n_fft, M, K - 1>
        wv = n_fft // 256
        for pairs in (2, 3, 4, 0, 64):
            run = 2 * (pairs or 2) - 1
            plan = ((run, 0), (wv * run, 70), (wv * run + 1, 0), (wv * run + 1, 128), (2 * wv * run, 0)) if pairs != 64 else ((run, 0), (run + 1, 75))
            for n_seg, rem in plan:
                M, K = WIDE_ISTFT[::-1][i % len(WIDE_ISTFT)] if pairs != 64 else (4, 2)
                add('apply_istft', M, K, n_fft, pairs, n_seg, rem, staged=(i % 3 == 0))
                i += 1
        for n_seg, rem in ((1, 114), (2, 0), (2, 128), (3, 0)):
            add('apply_istft', 4, 3, n_fft, 2, n_seg, rem)
        add('apply_istft', 4, 4, n_fft, 2, 14, 0, lengths=[(8, 94), (3 * wv, 0), (1, 99)])
    return cases


def _istft_inputs(c, R):
    """-> args of the fused call, the exact yf (R, K, T, F) float64."""
    M, K, n_fft, L = c['M'], c['K'], c['n_fft'], c['L']
    hop, F = n_fft // 2, n_fft // 2 + 1
    T = 1 + L // hop
    seed = _seed(M, K, n_fft, L, c['pairs'], 61)
    frames = None if c['lengths'] is None else [1 + l // hop for l in c['lengths']]
    if c['entry'] == 'istft':
        yf = spectra(np.random.default_rng(seed), (R, K, T, F), dither=True)
        args = (yf,)
    elif c['entry'] == 'step2_istft':
        args = onchip_scene(seed, R, K, M, T, F, dither=True)
    else:
        args = apply_scene(seed, R, K, M, T, F, dither=True)
    if frames is not None:
        for a in (args[0], args[1]) if c['entry'] == 'apply_istft' else (args[0],):
            for r in range(R):
                a[r, :, frames[r]:] = 0
    if c['entry'] == 'istft':
        ref = args[0].astype(np.complex128)
    elif c['entry'] == 'step2_istft':
        ref = ref_onchip(*args, q=16)[1]
    else:
        ref = ref_apply(args[0], args[1], args[2], q=16)
    return args, ref


def check_istft_case(make_engine, c):
    """One case of `istft_cases` -> (kernel name, the ratios quantity / restatement's quantity over every live segment).  Asserts every
    (room, node, hop segment) inside BAR_FACTOR x the restatement's quantity there, exact zeros beyond a room's length."""
    M, K, n_fft, L, lengths = c['M'], c['K'], c['n_fft'], c['L'], c['lengths']
    hop = n_fft // 2
    R = 2 if lengths is None else len(lengths)
    name = route(M, K, n_fft, c['entry'])[0]
    what = f'{name} {({k: v for k, v in c.items() if k not in ("entry",)})}'
    args, yf = _istft_inputs(c, R)
    yc = yf.astype(np.complex64)
    assert np.array_equal(yc.astype(np.complex128), yf)
    ref = room_wise(istft_f64, yf, L, n_fft, lengths)
    assert_segments_comparable(ref, hop, lengths)
    bar = BAR_FACTOR * segment_quantity(room_wise(istft_f32, yc, L, n_fft, lengths), ref, hop, lengths)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=n_fft, pad_mode='constant' if lengths is not None or L <= hop else 'reflect')
    try:
        assert eng.T == yf.shape[2]
        if c['pairs']:
            eng.set_tuning(istft_pairs=c['pairs'])
        if lengths is not None:
            eng.set_lengths(lengths)

        def staged_istft(spec):
            return eng.istft(spec.reshape(R * K, eng.T, eng.F)).numpy().reshape(R, K, L)
        if c['entry'] == 'istft':
            out, staged = staged_istft(eng.to_device(args[0], np.complex64)[1]), None
        elif c['entry'] == 'step2_istft':
            out = eng.step2_apply_istft_fused(*args).numpy()
            staged = staged_istft(eng.step2_apply_fused(*args)[0]) if c['staged'] else None
        else:
            X, Z, w = args
            res = eng.apply_istft(X, w, Z)
            assert res is not None, what + ': refused'
            out = res.numpy().reshape(R, K, L)
            staged = staged_istft(eng.apply(X, w, Z=Z)) if c['staged'] else None
    finally:
        eng.close()
    q = segment_quantity(out, ref, hop, lengths)
    bad = ~(q <= bar)
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} hop segments outside {BAR_FACTOR:g} x the float32 restatement; first (room, node, '
                           f'segment) {tuple(int(v) for v in np.argwhere(bad)[0])}: {q[bad][0]:.3e} against a bar of {bar[bad][0]:.3e}')
    if lengths is not None:
        for r, Lr in enumerate(lengths):
            assert not _bits(np.ascontiguousarray(out[r, :, Lr:])).any(), f'{what}: room {r} is not exactly 0 beyond its length'
    if staged is not None:                                               # the fused kernel against the two staged calls: the same bar
        qs = segment_quantity(out, ref, hop, lengths, against=staged)
        bad = ~(qs <= bar)
        assert not bad.any(), f'{what}: {int(bad.sum())} hop segments away from the staged calls by more than the bar; first {np.argwhere(bad)[0]}'
    live = bar > 0
    return name, (q[live] / (bar[live] / BAR_FACTOR))


def check_istft_cases(make_engine, cases):
    """-> {kernel family: {'worst': .., 'median': .., 'segments': ..}} of the ratio kernel's quantity / restatement's quantity."""
    ratios = {}
    for c in cases:
        name, r = check_istft_case(make_engine, c)
        ratios.setdefault(name.split('<')[0] + '<' + name.split('<')[1].split(',')[0] + '>', []).append(r)
    return {k: {'worst': float(np.max(np.concatenate(v))), 'median': float(np.median(np.concatenate(v))), 'segments': int(np.concatenate(v).size)}
            for k, v in ratios.items()}


def check_istft_nonfinite(make_engine, n_seg=17, t0=8):
    """A NaN in ONE frame of one signal's spectrum: every other signal is bit-identical to the clean run, and so are the hop segments of
    its own signal more than two frames away.  Frame t0 feeds segments t0 - 1 and t0; the frame it shares an inverse transform with
    (t0 - 1 or t0 + 1, depending on where the run starts) is spoilt with it and feeds one segment more on its side: segments
    t0 - 2 .. t0 + 1 may differ, nothing else.  For the kernel that forms z on chip the NaN reaches every node of its room through z at
    that frame; for a z row of the wide kernel every node but the row's own."""
    R, hop, F = 2, 256, 257
    L = n_seg * hop
    T = 1 + L // hop
    r0, f0 = 1, 100

    def run(entry, M, K, call, poison):
        args = list(_istft_inputs(dict(entry=entry, M=M, K=K, n_fft=512, L=L, pairs=3, lengths=None), R)[0])
        eng = make_engine(rooms=R, nodes=K, mics=M, length=L, n_fft=512)
        try:
            eng.set_tuning(istft_pairs=3)
            clean = call(eng, args)
            for which, idx, nodes in poison:
                hit_args = [a.copy() for a in args]
                hit_args[which][idx] = np.nan
                hit = call(eng, hit_args)
                same = same_bits(clean, hit)
                free = np.ones(clean.shape, bool)
                for k in nodes:
                    free[r0, k, max(0, t0 - 2) * hop:(t0 + 2) * hop] = False
                assert same[free].all(), f'{entry}: a NaN in frame {t0} moved {int((~same & free).sum())} samples it cannot reach'
                for k in nodes:
                    assert not np.isfinite(hit[r0, k, (t0 - 1) * hop:(t0 + 1) * hop]).any(), f'{entry}: the NaN did not reach node {k}'
        finally:
            eng.close()
    run('istft', 1, 2, lambda e, a: e.istft(a[0].reshape(R * 2, T, F)).numpy().reshape(R, 2, L), [(0, (r0, 1, t0, f0), (1,))])
    run('step2_istft', 2, 3, lambda e, a: e.step2_apply_istft_fused(*a).numpy(), [(0, (r0, 1, t0, f0, 0), (0, 1, 2))])
    run('apply_istft', 4, 3, lambda e, a: e.apply_istft(a[0], a[2], a[1]).numpy().reshape(R, 3, L),
        [(0, (r0, 1, t0, f0, 2), (1,)), (1, (r0, 2, t0, f0), (0, 1))])


def trace_names(text):
    """Kernel names of a kernel-trace summary (one per line, '#' comments) in the form `route` writes."""
    return {kernel_key(l) for l in text.splitlines() if l.strip() and not l.startswith('#')}
