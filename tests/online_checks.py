"""Checks of the online / adaptive MWF kernels (csrc/k_online.h: k_online_mwf_thread<P, SQ32>, k_online_mwf<P>) at every pencil size,
route and edge, through the staged call Engine.online_mwf (disco_online_mwf) on exactly known inputs.

Shared by tests/test_gpu_online_sizes.py (real MI355X, `-m gpu`), tests/test_online_sizes_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut down) and tests/test_online_sizes_cpu.py (the reference side alone: where the bars come from).
`make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library under test.

Route table of the online mode (api_online.hip), every instantiated kernel is launched by check_sizes:
    P = 1 .. 4     k_online_mwf_thread<1..4>            always ("online_sq32" 1 / 0: packed-float32 / float64 squarings)
    P = 5 .. 7     k_online_mwf_thread<5>, <6>, <7>     while "solve_thread" = 1 (default); "online_sq32" as above
                   k_online_mwf<5>, <6>, <7>            when "solve_thread" = 0 (8 lanes per problem, 16 problems per block)
    P = 8          k_online_mwf<8>                      8 lanes per problem
    P = 9 .. 16    k_online_mwf<9>, <10>, <11>, <12>, <13>, <14>, <15>, <16>       16 lanes per problem, 4 problems per block
    P > 16         refused (DISCO_E_UNSUPPORTED)

THE REFERENCE of every value check is oracle/online_oracle.py:online_mwf (float64; pinned on the reference's own functions by
tests/golden/online_ref.npz).  Every (room, node, bin) problem is compared on its own, in three quantities:
    series   || out[:, f] - ref ||_2 / || ref ||_2 over t
    frame    max_t | out - ref | / max_t | ref |          (one wrong frame is not averaged away)
    w        || w_last - ref || / || ref || over the P entries of the filter in force at the last frame

THE BAR.  The kernels keep both smoothed matrices in float32, so their distance from the float64 oracle depends on P and on the
conditioning of the scene.  It is measured on the reference side alone: `online_mwf_f32state` below restates the oracle with Rss, Rnn,
the products and out rounded to float32 / complex64 every frame (the solve stays mwf_oracle.gevd_mwf_r1_hermitian in float64; plain
NumPy, no kernel code), and `DIST` records, per scene variant, per P and per quantity, the worst per-problem distance between that
restatement and the oracle over every input the checks use at that P.  A check passes when the kernel is within BAR_FACTOR = 4 times
that distance: the kernel and the restatement are two independent float32 roundings of one recursion (x 2: the distance between two
realisations instead of one realisation and the exact value), times 2 for the spread between seeds.  tests/test_online_sizes_cpu.py
recomputes DIST with `recompute_dist` and asserts that the committed figures are not smaller than what it finds and not more than
twice as large.  A cut-down run (the emulator: one room, a prefix of the frames; the walk is causal, so a prefix is a case of its
own) measures the same distance on its own inputs at run time, with the same factor.  The committed figures are what
`recompute_dist` printed, times 1.1 and rounded up to two digits (LAPACK builds differ in the last bits).

Scene (well conditioned by construction, so that the bar means something): per room one source with a random steering vector over
all channels, on or off per frame, plus white noise of unit variance on every row; masks 0.9 / 0.1 following the source activity with
jitter.  In the step-2 form the exchanged z rows are channels of the same scene, distinct per node (a swapped pair of rows fails).
"""
import zlib

import numpy as np

from oracle import mwf_oracle as mo
from oracle import online_oracle as oo

N_FFT = 512
HOP = 256
F_BINS = 257
BAR_FACTOR = 4.0
QUANT = ('series', 'frame', 'w')


def f32(x):
    """The float32 value the C ABI receives, as a Python float: the oracle gets the parameters the kernel gets."""
    return float(np.float32(x))


# ---- the scene ---------------------------------------------------------------------------------------------------------------------

def scene(seed, R, K, M, T, step2, mask_mode='soft'):
    """-> X (R, K, T, F, M) c64, Z (R, K, T, F) c64 or None, mask (R, K, T, F) f32.  mask_mode: 'soft' 0.9 / 0.1 + jitter, 'binary'
    exactly 1 / 0 following the activity, 'ones', 'zeros'."""
    rng = np.random.default_rng(seed)
    F = F_BINS
    C_ = K * M + (K if step2 else 0)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    act = rng.integers(0, 2, (R, T)).astype(np.float64)
    act[:, 0] = 1.0                                                   # the very first solve sees the source
    steer = cn(R, 1, F, C_)
    src = 2.0 * cn(R, T, F, 1) * act[:, :, None, None]
    v = (steer * src + cn(R, T, F, C_)).astype(np.complex64)          # (R, T, F, C)
    X = np.ascontiguousarray(v[..., :K * M].reshape(R, T, F, K, M).transpose(0, 3, 1, 2, 4))
    Z = np.ascontiguousarray(v[..., K * M:].transpose(0, 3, 1, 2)) if step2 else None
    jit = rng.uniform(-0.05, 0.05, (R, K, T, F))
    a = act[:, None, :, None]
    if mask_mode == 'soft':
        mask = 0.1 + 0.8 * a + jit
    elif mask_mode == 'binary':
        mask = a + 0.0 * jit
    elif mask_mode == 'ones':
        mask = np.ones_like(jit)
    elif mask_mode == 'zeros':
        mask = np.zeros_like(jit)
    else:
        raise ValueError(mask_mode)
    return X, Z, np.ascontiguousarray(mask.astype(np.float32))


def problems(X, Z, mask, nodes=None):
    """The kernel's problems in its own order (room, node, bin): V (P, n, T) with rows [X_k ; z_j, j < k ; z_j, j > k]
    (tango.py:142-155), mask (n, T).  nodes: the global node indices held (X / mask carry all K)."""
    R, K, T, F, M = X.shape
    nodes = range(K) if nodes is None else nodes
    Vs, ms = [], []
    for r in range(R):
        for k in nodes:
            rows = [X[r, k].transpose(2, 1, 0)]                                          # (M, F, T)
            if Z is not None:
                rows += [Z[r, j].T[None] for j in range(K) if j < k] + [Z[r, j].T[None] for j in range(K) if j > k]
            Vs.append(np.concatenate(rows, 0))
            ms.append(mask[r, k].T)
    return np.concatenate(Vs, 1), np.concatenate(ms, 0)


# ---- the reference and its float32-state restatement -------------------------------------------------------------------------------

def online_mwf_f32state(V, mask, lambda_cor=0.95, mu=1.0, update_every=1, init_diag=1e-3):
    """oracle/online_oracle.py:online_mwf with the STATE in float32: Rss, Rnn, the outer products, their weights and out are rounded to
    float32 / complex64 at every frame; the solve is the oracle's float64 closed form on those matrices.  V (P, n, T), mask (n, T) ->
    out (n, T) c64, w_last (n, P) c64."""
    V = np.asarray(V, dtype=np.complex64)
    mask = np.asarray(mask, dtype=np.float32)
    P, n, T = V.shape
    lam = np.float32(lambda_cor)
    oml = np.float32(1.0) - lam
    Rss = np.zeros((n, P, P), np.complex64)
    Rnn = np.tile((np.float32(init_diag) * np.eye(P, dtype=np.float32)).astype(np.complex64), (n, 1, 1))
    w = np.zeros((n, P), np.complex64)
    out = np.zeros((n, T), np.complex64)
    for t in range(T):
        v = np.ascontiguousarray(V[:, :, t].T)
        vv = v[:, :, None] * np.conjugate(v)[:, None, :]
        m = mask[:, t]
        cs = (oml * m)[:, None, None]
        cn = (oml * (np.float32(1.0) - m))[:, None, None]
        Rss = lam * Rss + cs * vv
        Rnn = lam * Rnn + cn * vv
        assert Rss.dtype == np.complex64 and Rnn.dtype == np.complex64
        if t % update_every == 0:
            w = mo.gevd_mwf_r1_hermitian(Rss, Rnn, mu)[0].astype(np.complex64)
        out[:, t] = np.einsum('np,np->n', np.conjugate(w), v)
    return out, w


def distances(out, w, ref_out, ref_w):
    """Per problem: out (n, T), w (n, P) against the reference -> dict of (n,) arrays, keys QUANT."""
    out, w = np.asarray(out, np.complex128), np.asarray(w, np.complex128)
    d = np.abs(out - ref_out)
    return {'series': np.linalg.norm(out - ref_out, axis=1) / np.maximum(np.linalg.norm(ref_out, axis=1), 1e-300),
            'frame': d.max(axis=1) / np.maximum(np.abs(ref_out).max(axis=1), 1e-300),
            'w': np.linalg.norm(w - ref_w, axis=1) / np.maximum(np.linalg.norm(ref_w, axis=1), 1e-300)}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

# (M, K) of the step-2 form: every P2 = M + K - 1 = 2 .. 16 at least once; K = 9 with M = 8; M = 1 with K = 16; K >= 6 (2, 6), (6, 6)
STEP2_SHAPES = ((1, 2), (2, 2), (2, 3), (3, 3), (2, 5), (2, 6), (4, 5), (8, 2), (8, 3), (6, 6), (8, 5), (8, 6), (8, 7), (8, 8), (8, 9),
                (1, 16))
STEP1_SIZES = tuple(range(1, 17))
EDGE_SIZES = (1, 4, 7, 8, 16)
SCHEDULE_SIZES = (3, 8, 13)              # one per kernel geometry: thread, 8 lanes, 16 lanes
T_MAIN, T_SCHED, T_ONES = 20, 12, 40
SCHEDULES = {'u1': 1, 'u2': 2, 'u3': 3, 'uTm1': T_SCHED - 1, 'uT': T_SCHED, 'uTp5': T_SCHED + 5}

# scene variants: name -> (parameters of the call, mask mode, frames)
VARIANTS = {
    'd1': (dict(lambda_cor=0.95, mu=1.0, update_every=3, init_diag=1.0), 'soft', T_MAIN),
    'd1e-3': (dict(lambda_cor=0.95, mu=1.0, update_every=3, init_diag=1e-3), 'soft', T_MAIN),       # the shipped default init_diag
    'ones': (dict(lambda_cor=0.95, mu=1.0, update_every=3, init_diag=1.0), 'ones', T_ONES),         # Rnn = lambda^t init_diag I exactly
    'binary': (dict(lambda_cor=0.95, mu=1.0, update_every=3, init_diag=1.0), 'binary', T_MAIN),
    'lam999': (dict(lambda_cor=0.999, mu=1.0, update_every=3, init_diag=1.0), 'soft', T_MAIN),
    'mu0.3': (dict(lambda_cor=0.95, mu=0.3, update_every=3, init_diag=1.0), 'soft', T_MAIN),
    'mu10': (dict(lambda_cor=0.95, mu=10.0, update_every=3, init_diag=1.0), 'soft', T_MAIN),
}
for _n, _u in SCHEDULES.items():
    VARIANTS[_n] = (dict(lambda_cor=0.95, mu=1.0, update_every=_u, init_diag=1.0), 'soft', T_SCHED)
R_FULL = 2


class Case:
    """One input of the checks: a scene variant at one shape.  K = 1: the step-1 form (nodes = 1, mics = P, Z = None); K > 1: the step-2
    form (P = M + K - 1, Z given).  cut = (rooms, frames): a prefix of the full case (rooms are independent, the walk is causal)."""

    def __init__(self, variant, M, K, cut=None):
        self.variant, self.M, self.K, self.cut = variant, M, K, cut
        self.params, self.mask_mode, self.T_full = VARIANTS[variant]
        self.P = M if K == 1 else M + K - 1
        self.seed = zlib.crc32(f'{variant}/{M}/{K}'.encode())
        self.R, self.T = (R_FULL, self.T_full) if cut is None else (min(cut[0], R_FULL), min(cut[1], self.T_full))
        self._in = self._ref = None

    def inputs(self):
        if self._in is None:
            X, Z, mask = scene(self.seed, R_FULL, self.K, self.M, self.T_full, self.K > 1, self.mask_mode)
            if self.cut is not None:
                X, mask = np.ascontiguousarray(X[:self.R, :, :self.T]), np.ascontiguousarray(mask[:self.R, :, :self.T])
                Z = None if Z is None else np.ascontiguousarray(Z[:self.R, :, :self.T])
            self._in = (X, Z, mask)
        return self._in

    def oracle_params(self):
        p = self.params
        return dict(lambda_cor=f32(p['lambda_cor']), mu=f32(p['mu']), update_every=p['update_every'], init_diag=f32(p['init_diag']))

    def reference(self):
        """float64 oracle on every problem: ref_out (n, T), ref_w (n, P)."""
        if self._ref is None:
            V, m = problems(*self.inputs())
            out, w_all = oo.online_mwf(V, m, **self.oracle_params())
            self._ref = (out, w_all[:, -1])
        return self._ref

    def restatement_distance(self):
        """Worst per-problem distance of the float32-state restatement from the oracle on this case's inputs: {quantity: float}."""
        V, m = problems(*self.inputs())
        out, w = online_mwf_f32state(V, m, **self.oracle_params())
        d = distances(out, w, *self.reference())
        return {q: float(d[q].max()) for q in QUANT}

    def bar(self):
        """{quantity: bar}: the committed table for a full case, measured on the spot for a cut one."""
        if self.cut is None:
            d = dict(zip(QUANT, DIST[self.variant][self.P]))
        else:
            d = self.restatement_distance()
        return {q: BAR_FACTOR * d[q] for q in QUANT}


_cases = {}


def case(variant, M, K, cut=None):
    key = (variant, M, K, cut)
    if key not in _cases:
        _cases[key] = Case(variant, M, K, cut)
    return _cases[key]


def table_cases():
    """Every full case the checks take a bar from: variant -> list of (M, K)."""
    main = [(P, 1) for P in STEP1_SIZES] + list(STEP2_SHAPES)
    t = {'d1': main, 'd1e-3': main}
    for v in ('ones', 'binary', 'lam999', 'mu0.3', 'mu10'):
        t[v] = [(P, 1) for P in EDGE_SIZES]
    for v in SCHEDULES:
        t[v] = [(P, 1) for P in SCHEDULE_SIZES]
    return t


def recompute_dist(variants=None, verbose=False):
    """The table DIST from scratch: variant -> {P: (series, frame, w)}, the worst restatement-vs-oracle distance over the cases at that P."""
    res = {}
    for v, shapes in table_cases().items():
        if variants is not None and v not in variants:
            continue
        res[v] = {}
        for M, K in shapes:
            c = Case(v, M, K)                                       # not cached: the table run would hold every reference at once
            d = c.restatement_distance()
            old = res[v].get(c.P, (0.0, 0.0, 0.0))
            res[v][c.P] = tuple(max(o, d[q]) for o, q in zip(old, QUANT))
            if verbose:
                print(v, (M, K), c.P, d, flush=True)
    return res


def round_up(x, headroom=1.1):
    """x * headroom rounded up to two significant digits (how the committed table is written)."""
    x *= headroom
    e = int(np.floor(np.log10(x))) - 1
    return float(f'{np.ceil(x / 10.0 ** e) * 10.0 ** e:.1e}')


# Worst per-problem distance between online_mwf_f32state and the float64 oracle: variant -> {P: (series, frame, w)}.  Written by
#   python -c "import online_checks as oc; oc.print_dist()"       (in tests/)
# and checked against a recomputation by tests/test_online_sizes_cpu.py.  The bar of a check is BAR_FACTOR times its entry.
DIST = {
    'd1': {
        1: (2.2e-07, 2.9e-07, 3.2e-07),
        2: (5.8e-07, 7.8e-07, 8.4e-07),
        3: (3.3e-07, 4.2e-07, 1.1e-06),
        4: (4.5e-07, 7.9e-07, 6.3e-07),
        5: (4.6e-07, 5.9e-07, 8.8e-07),
        6: (2.5e-07, 2.8e-07, 1.1e-06),
        7: (3.3e-07, 4.4e-07, 5.3e-06),
        8: (6.3e-07, 9.5e-07, 1.6e-06),
        9: (2.0e-07, 3.1e-07, 1.5e-06),
        10: (2.0e-07, 2.8e-07, 8.5e-07),
        11: (3.1e-07, 3.7e-07, 9.9e-07),
        12: (4.0e-07, 4.2e-07, 9.7e-07),
        13: (2.0e-07, 3.2e-07, 1.1e-06),
        14: (1.7e-07, 2.5e-07, 1.1e-06),
        15: (2.2e-07, 4.1e-07, 1.1e-06),
        16: (2.4e-07, 3.1e-07, 1.9e-06),
    },
    'd1e-3': {
        1: (1.7e-07, 2.4e-07, 1.8e-07),
        2: (1.5e-05, 2.7e-05, 3.6e-06),
        3: (1.3e-05, 1.6e-05, 2.9e-06),
        4: (2.1e-05, 3.7e-05, 5.9e-06),
        5: (5.9e-05, 1.2e-04, 1.3e-05),
        6: (3.9e-05, 6.2e-05, 9.7e-06),
        7: (7.0e-05, 7.7e-05, 5.2e-05),
        8: (6.7e-05, 1.3e-04, 4.8e-04),
        9: (8.1e-05, 1.2e-04, 3.6e-04),
        10: (8.9e-05, 1.7e-04, 1.6e-04),
        11: (1.5e-04, 1.9e-04, 3.8e-04),
        12: (1.8e-04, 2.1e-04, 3.8e-04),
        13: (2.2e-04, 3.2e-04, 4.6e-04),
        14: (1.7e-04, 2.6e-04, 9.0e-04),
        15: (3.4e-04, 5.5e-04, 1.4e-03),
        16: (3.1e-04, 5.6e-04, 1.6e-03),
    },
    'ones': {
        1: (8.4e-08, 1.3e-07, 6.6e-08),
        4: (2.8e-07, 4.4e-07, 5.9e-07),
        7: (1.6e-07, 2.6e-07, 5.4e-07),
        8: (1.8e-07, 2.6e-07, 2.5e-07),
        16: (1.6e-07, 2.3e-07, 6.3e-07),
    },
    'binary': {
        1: (2.0e-07, 2.8e-07, 2.3e-07),
        4: (4.5e-07, 5.2e-07, 2.8e-06),
        7: (2.4e-07, 2.8e-07, 3.8e-07),
        8: (1.6e-07, 2.4e-07, 2.8e-07),
        16: (1.6e-07, 2.3e-07, 8.0e-07),
    },
    'lam999': {
        1: (4.0e-07, 5.0e-07, 4.9e-07),
        4: (3.6e-07, 4.2e-07, 5.7e-07),
        7: (2.5e-07, 3.2e-07, 4.6e-07),
        8: (2.8e-07, 3.2e-07, 7.9e-07),
        16: (1.9e-07, 3.1e-07, 3.7e-07),
    },
    'mu0.3': {
        1: (1.4e-07, 1.9e-07, 1.6e-07),
        4: (2.9e-07, 3.9e-07, 7.0e-07),
        7: (1.8e-07, 2.6e-07, 6.9e-07),
        8: (1.5e-07, 2.2e-07, 7.7e-07),
        16: (1.6e-07, 2.7e-07, 8.0e-07),
    },
    'mu10': {
        1: (4.8e-07, 5.4e-07, 5.5e-07),
        4: (5.6e-07, 6.8e-07, 5.7e-07),
        7: (2.0e-07, 2.6e-07, 8.5e-07),
        8: (1.6e-07, 2.6e-07, 9.6e-07),
        16: (2.1e-07, 3.0e-07, 6.5e-07),
    },
    'u1': {
        3: (2.0e-07, 3.2e-07, 5.4e-07),
        8: (1.4e-07, 1.9e-07, 4.0e-07),
        13: (1.9e-07, 2.6e-07, 3.8e-07),
    },
    'u2': {
        3: (3.1e-07, 4.8e-07, 1.2e-06),
        8: (1.8e-07, 2.4e-07, 1.5e-06),
        13: (1.7e-07, 2.4e-07, 5.0e-07),
    },
    'u3': {
        3: (6.0e-07, 8.8e-07, 1.3e-06),
        8: (1.9e-07, 2.3e-07, 4.6e-07),
        13: (1.7e-07, 2.3e-07, 6.0e-07),
    },
    'uTm1': {
        3: (3.9e-07, 5.4e-07, 7.1e-07),
        8: (3.6e-07, 7.0e-07, 4.6e-07),
        13: (2.2e-07, 2.9e-07, 5.5e-07),
    },
    'uT': {
        3: (1.5e-07, 2.3e-07, 1.3e-07),
        8: (1.3e-07, 1.8e-07, 9.7e-08),
        13: (1.7e-07, 2.1e-07, 7.6e-08),
    },
    'uTp5': {
        3: (1.5e-07, 1.9e-07, 1.3e-07),
        8: (1.3e-07, 1.8e-07, 1.3e-07),
        13: (1.5e-07, 2.2e-07, 1.1e-07),
    },
}


def print_dist():
    t = recompute_dist(verbose=True)
    print('DIST = {')
    for v, rows in t.items():
        print(f'    {v!r}: {{')
        for P in sorted(rows):
            print(f'        {P}: ({", ".join(f"{round_up(x):.1e}" for x in rows[P])}),')
        print('    },')
    print('}')


# ---- driving the kernel -------------------------------------------------------------------------------------------------------------

def routes(P):
    """Every kernel route that serves P: (name, options)."""
    if P <= 4:
        return [('thread', {'online_sq32': 1}), ('thread_sq64', {'online_sq32': 0})]
    if P <= 7:
        return [('thread', {'solve_thread': 1, 'online_sq32': 1}), ('thread_sq64', {'solve_thread': 1, 'online_sq32': 0}),
                ('group', {'solve_thread': 0})]
    return [('group', {})]


def z_blocks(Z, blk):
    """[R][K] planes -> the rank-major layout [K / blk][R][blk] (what an all-gather over K / blk ranks delivers)."""
    R, K = Z.shape[:2]
    return np.ascontiguousarray(Z.reshape(R, K // blk, blk, *Z.shape[2:]).swapaxes(0, 1))


def run_kernel(make_engine, X, Z, mask, K, params, options=None, shard=None, zblk=None):
    """Engine.online_mwf on the given inputs -> out (n, T), w_last (n, P) in problem order (room, node, bin).
    shard = (k0, Kl): the engine holds those nodes only (X / mask are cut here, Z keeps all K)."""
    R, _, T, F, M = X.shape
    eng = make_engine(rooms=R, nodes=K, mics=M, length=(T - 1) * HOP, n_fft=N_FFT)
    assert (eng.T, eng.F) == (T, F), (eng.T, eng.F)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    if shard is not None:
        k0, Kl = shard
        eng.set_node_shard(k0, Kl)
        X, mask = np.ascontiguousarray(X[:, k0:k0 + Kl]), np.ascontiguousarray(mask[:, k0:k0 + Kl])
    if zblk is not None:
        eng.set_z_blocks(zblk)
        Z = z_blocks(Z, zblk)
    out, w = eng.online_mwf(X, mask, Z=Z, want_w=True, **params)
    out, w = out.numpy(), w.numpy()
    eng.close()
    n = out.shape[0] * out.shape[1] * F
    return np.ascontiguousarray(out.transpose(0, 1, 3, 2)).reshape(n, T), w.reshape(n, -1)


def _worst(d):
    return {q: float(d[q].max()) for q in QUANT}


def _assert_within(d, bar, what):
    """Every problem within the bar in every quantity; names the worst problem."""
    for q in QUANT:
        i = int(np.argmax(d[q]))
        assert np.isfinite(d[q]).all() and d[q][i] <= bar[q], (what, q, 'problem', i, float(d[q][i]), 'bar', bar[q])


def _note(seen, P, route, w):
    cur = seen.setdefault(P, {}).setdefault(route, dict.fromkeys(QUANT, 0.0))
    for q in QUANT:
        cur[q] = max(cur[q], w[q])


def compare_case(make_engine, c, route_list=None, seen=None, **run):
    """Run case c on every route (or those named) and compare every problem and frame with the oracle."""
    X, Z, mask = c.inputs()
    ref_out, ref_w = c.reference()
    bar = c.bar()
    if run.get('shard') is not None:
        k0, Kl = run['shard']
        n1 = F_BINS
        sel = np.concatenate([np.arange((r * c.K + k) * n1, (r * c.K + k + 1) * n1) for r in range(c.R) for k in range(k0, k0 + Kl)])
        ref_out, ref_w = ref_out[sel], ref_w[sel]
    for name, opts in routes(c.P):
        if route_list is not None and name not in route_list:
            continue
        out, w = run_kernel(make_engine, X, Z, mask, c.K, c.params, options=opts, **run)
        assert np.isfinite(out.view(np.float32)).all() and np.isfinite(w.view(np.float32)).all(), (c.variant, c.M, c.K, name)
        d = distances(out, w, ref_out, ref_w)
        wv = _worst(d)
        print(f'online {c.variant} M={c.M} K={c.K} P={c.P} {name} {run if run else ""}: ' + ' '.join(f'{q}={wv[q]:.2e}/{bar[q]:.2e}' for q in QUANT),
              flush=True)
        if seen is not None:
            _note(seen, c.P, name, wv)
        _assert_within(d, bar, (c.variant, c.M, c.K, name, run))


# ---- check 1: every size against the oracle ---------------------------------------------------------------------------------------

def check_sizes(make_engine, variant='d1', step1=STEP1_SIZES, step2=STEP2_SHAPES, cut=None):
    """P = 1 .. 16 in the step-1 form (an engine with nodes = 1, mics = P: disco_create does not limit mics and the staged call needs no
    transform) and every step-2 shape, every route.  R = 2 rooms of 257 bins: in the step-1 form of every P (and in most step-2 shapes)
    n_prob = R Kl 257 is no multiple of the 16 or 4 problems of a block, so the dead-group path runs at every size.  -> {P: {route: {quantity: worst}}}"""
    seen = {}
    for M, K in [(P, 1) for P in step1] + list(step2):
        compare_case(make_engine, case(variant, M, K, cut), seen=seen)
    return seen


# ---- check 2: the update schedule ---------------------------------------------------------------------------------------------------

def check_schedule(make_engine, sizes=SCHEDULE_SIZES, cut=None):
    """update_every in {1, 2, 3, T - 1, T, T + 5}.  With U >= T the filter of frame 0 stays in force: the very first solve (Rnn =
    lambda init_diag I + one outer product) is pinned frame by frame, and w_last is the frame-0 filter."""
    seen = {}
    for name, U in SCHEDULES.items():
        for P in sizes:
            c = Case(name, P, 1, cut)
            if U >= c.T:                                        # the reference side says what this case pins
                V, m = problems(*c.inputs())
                w_all = oo.online_mwf(V, m, **c.oracle_params())[1]
                assert np.array_equal(w_all[:, -1], w_all[:, 0])
            compare_case(make_engine, c, route_list=('thread', 'group'), seen=seen.setdefault(name, {}))
    return seen


# ---- check 3: row order and z layout -----------------------------------------------------------------------------------------------

def check_row_order(make_engine, shapes=((2, 6, 3), (8, 9, 3)), variant='d1', cut=None, every_k0=True):
    """(a) a node shard (k0, Kl = 1) for every k0 and one Kl = 2 shard against the oracle rows [Y_k ; z_j, j < k ; z_j, j > k] with z
    distinct per node; (b) the same calls with Z in rank-major blocks (set_z_blocks): bit-identical to the plain [R][K] layout.
    shapes: (M, K, nodes per z block); every_k0 = False (the emulator): first, middle and last node only."""
    seen = {}
    for M, K, blk in shapes:
        c = case(variant, M, K, cut)
        X, Z, mask = c.inputs()
        rl = ('thread', 'group')
        for shard in [(k0, 1) for k0 in (range(K) if every_k0 else (0, K // 2, K - 1))] + [(K // 2 - 1, 2)]:
            compare_case(make_engine, c, route_list=rl, seen=seen, shard=shard)
        for name, opts in routes(c.P):
            if name not in rl:
                continue
            for shard in (None, (K // 2 - 1, 2), (K - 1, 1), (0, 1)):
                plain = run_kernel(make_engine, X, Z, mask, K, c.params, options=opts, shard=shard)
                for b in sorted({blk, K // blk}):
                    blocked = run_kernel(make_engine, X, Z, mask, K, c.params, options=opts, shard=shard, zblk=b)
                    assert np.array_equal(plain[0].view(np.uint32), blocked[0].view(np.uint32)), (M, K, name, shard, b)
                    assert np.array_equal(plain[1].view(np.uint32), blocked[1].view(np.uint32)), (M, K, name, shard, b)
    return seen


# ---- check 5: mask and parameter edges ---------------------------------------------------------------------------------------------

def check_edges(make_engine, sizes=EDGE_SIZES, cut=None):
    """mask == 1 (T = 40), masks of exactly 0 and 1, lambda = 0.999, mu 0.3 and 10 against the oracle (init_diag 1 and 1e-3: variants
    'd1' and 'd1e-3' of check_sizes); mask == 0: finite and |w_last| < 1e-12 (Rss stays 0: check_solver_degenerate's statement);
    lambda = 0: singular Rnn from frame 1 on, finite and below the 1e4 of gevd_rank_checks.check_degenerate."""
    seen = {}
    for P in sizes:
        for v in ('ones', 'binary', 'lam999', 'mu0.3', 'mu10'):
            compare_case(make_engine, Case(v, P, 1, cut), seen=seen.setdefault(v, {}))
        c = Case('d1', P, 1, cut)
        X, _, _ = c.inputs()
        vmax = float(np.abs(X).max())
        for name, opts in routes(P):
            out, w = run_kernel(make_engine, X, None, np.zeros(X.shape[:4], np.float32), 1, c.params, options=opts)
            assert np.isfinite(out.view(np.float32)).all() and np.isfinite(w.view(np.float32)).all(), (P, name)
            assert float(np.abs(w).max()) < 1e-12, (P, name, float(np.abs(w).max()))
            out, w = run_kernel(make_engine, *c.inputs(), 1, dict(c.params, lambda_cor=0.0), options=opts)
            assert np.isfinite(out.view(np.float32)).all() and np.isfinite(w.view(np.float32)).all(), (P, name)
            assert float(np.abs(w).max()) < 1e4 and float(np.abs(out).max()) < 1e4 * P * vmax, (P, name, float(np.abs(w).max()))
    return seen


def check_refusals(make_engine):
    """Bad arguments return the documented error and leave `out` untouched (the C ABI directly: Engine.online_mwf derives P itself)."""
    E_ARG, E_UNSUPPORTED = -1, -2
    T = 4

    def call(eng, P, with_z, lam=0.95, U=1, init=1e-3):
        R, K, M, F = eng.R, eng.K, eng.M, eng.F
        rng = np.random.default_rng(5)
        X = (rng.standard_normal((R, K, T, F, M)) + 1j * rng.standard_normal((R, K, T, F, M))).astype(np.complex64)
        Z = (rng.standard_normal((R, K, T, F)) + 1j * rng.standard_normal((R, K, T, F))).astype(np.complex64)
        px, kx = eng.to_device(X, np.complex64)
        pz, kz = eng.to_device(Z if with_z else None, np.complex64)
        pm, km = eng.to_device(np.full((R, K, T, F), 0.5, np.float32), np.float32)
        sentinel = np.full((R, K, T, F), 7.0 - 3.0j, np.complex64)
        po, ko = eng.to_device(sentinel, np.complex64)
        rc = eng.lib.disco_online_mwf(eng.ctx, px, pz, pm, P, lam, 1.0, U, init, po, None, eng.stream)
        eng.sync()
        return rc, np.array_equal(ko.numpy(), sentinel), eng.lib.disco_last_error(eng.ctx).decode()
    eng = make_engine(rooms=1, nodes=3, mics=2, length=(T - 1) * HOP, n_fft=N_FFT)
    rc, untouched, _ = call(eng, 4, True)
    assert rc == 0 and not untouched                                      # the harness itself: a good call writes out
    for what, kw, want in (('lambda = 1', dict(P=4, with_z=True, lam=1.0), E_ARG), ('lambda < 0', dict(P=4, with_z=True, lam=-0.1), E_ARG),
                           ('lambda NaN', dict(P=4, with_z=True, lam=float('nan')), E_ARG),
                           ('update_every = 0', dict(P=4, with_z=True, U=0), E_ARG), ('init_diag = 0', dict(P=4, with_z=True, init=0.0), E_ARG),
                           ('P = 3', dict(P=3, with_z=True), E_ARG), ('P = 5', dict(P=5, with_z=True), E_ARG),
                           ('P > M without Z', dict(P=4, with_z=False), E_ARG)):
        rc, untouched, msg = call(eng, **kw)
        assert rc == want and untouched and 'disco_online_mwf' in msg, (what, rc, untouched, msg)
    eng.close()
    eng = make_engine(rooms=1, nodes=10, mics=8, length=(T - 1) * HOP, n_fft=N_FFT)          # P2 = 17
    rc, untouched, msg = call(eng, 17, True)
    assert rc == E_UNSUPPORTED and untouched and '16' in msg, (rc, untouched, msg)
    rc, untouched, _ = call(eng, 8, False)
    assert rc == 0 and not untouched                                      # step 1 of the same engine still runs
    eng.close()
    eng = make_engine(rooms=1, nodes=1, mics=17, length=(T - 1) * HOP, n_fft=N_FFT)
    rc, untouched, msg = call(eng, 17, False)
    assert rc == E_UNSUPPORTED and untouched, (rc, untouched, msg)
    eng.close()


# ---- check 6: non-finite input stays where it is ----------------------------------------------------------------------------------

def check_nonfinite(make_engine, sizes=EDGE_SIZES, step2=((2, 3), (2, 6), (4, 5), (8, 9)), cut=None):
    """One NaN (room 0, bin 0: the problem the dead groups walk too) and, separately, one inf (room 1 -- or 0 when cut --, bin 130) in X at
    frame t0 > 0: every other problem bit-identical to the clean run, and the poisoned problem's frames t < t0 too (the walk is causal).
    A NaN in one remote Z entry touches only that bin's problems in the nodes that receive that z."""
    F = F_BINS

    def same(a, b):
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for P in sizes:
        c = Case('d1', P, 1, cut)
        X, _, mask = c.inputs()
        t0 = c.T // 2
        for name, opts in routes(P):
            clean = run_kernel(make_engine, X, None, mask, 1, c.params, options=opts)
            for bad, r, f, ch in ((np.nan, 0, 0, 0), (np.inf, c.R - 1, 130, P - 1)):
                Xb = X.copy()
                Xb[r, 0, t0, f, ch] = bad
                out, w = run_kernel(make_engine, Xb, None, mask, 1, c.params, options=opts)
                pid = r * F + f
                keep = np.arange(out.shape[0]) != pid
                assert same(out[keep], clean[0][keep]) and same(w[keep], clean[1][keep]), (P, name, bad, 'neighbours moved')
                assert same(out[pid, :t0], clean[0][pid, :t0]), (P, name, bad, 'frames before t0 moved')
                assert not np.isfinite(out[pid, t0]), (P, name, bad, 'the poisoned frame is finite')
    for M, K in step2:
        c = case('d1', M, K, cut)
        X, Z, mask = c.inputs()
        t0, r, j, f = c.T // 2, c.R - 1, K // 2, 77
        for name, opts in routes(c.P):
            if name == 'thread_sq64':
                continue
            clean = run_kernel(make_engine, X, Z, mask, K, c.params, options=opts)
            Zb = Z.copy()
            Zb[r, j, t0, f] = np.nan
            out, w = run_kernel(make_engine, X, Zb, mask, K, c.params, options=opts)
            hit = np.array([(r * K + k) * F + f for k in range(K) if k != j])
            keep = np.ones(out.shape[0], bool)
            keep[hit] = False
            assert same(out[keep], clean[0][keep]) and same(w[keep], clean[1][keep]), (M, K, name, 'problems without that z moved')
            assert same(out[hit, :t0], clean[0][hit, :t0]), (M, K, name, 'frames before t0 moved')
            assert not np.isfinite(out[hit, t0]).any(), (M, K, name, 'a receiver of the poisoned z is finite')


# ---- check 7: the two routes of P = 5, 6, 7 against each other ---------------------------------------------------------------------

def check_routes(make_engine, sizes=(5, 6, 7), step2=((2, 6),), variant='d1', cut=None):
    """Thread route against group route on the same inputs: two mappings of one float32 recursion, held to the same table entry as
    either against the oracle (distances relative to the thread route's outputs)."""
    seen = {}
    for M, K in [(P, 1) for P in sizes] + list(step2):
        c = case(variant, M, K, cut)
        X, Z, mask = c.inputs()
        r = dict(routes(c.P))
        a = run_kernel(make_engine, X, Z, mask, K, c.params, options=r['thread'])
        b = run_kernel(make_engine, X, Z, mask, K, c.params, options=r['group'])
        d = distances(b[0], b[1], a[0].astype(np.complex128), a[1].astype(np.complex128))
        wv, bar = _worst(d), c.bar()
        print(f'online routes {variant} M={M} K={K} P={c.P} group vs thread: ' + ' '.join(f'{q}={wv[q]:.2e}/{bar[q]:.2e}' for q in QUANT), flush=True)
        _note(seen, c.P, 'group_vs_thread', wv)
        _assert_within(d, bar, ('routes', M, K))
    return seen
