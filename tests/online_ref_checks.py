"""Checks of the online / adaptive MWF with COMPANIONS (csrc/k_online_ref.h: k_online_mwf_thread_ref<P, SQ32>, k_online_mwf_ref<P>;
disco_online_mwf_ref, disco_tango_online_reference): the target and the noise image carried through the per-frame filters of the
mixture, which is what every score of the reference needs.

Shared by tests/test_gpu_online_ref.py (real MI355X, `-m gpu`), tests/test_online_ref_emulated.py (the same kernel sources under the
hipemu CPU emulator, cut down) and tests/test_online_ref_cpu.py (the reference side alone: where the bars come from).  Shapes, routes,
schedules, the problem order, the distance measures and BAR_FACTOR are those of tests/online_checks.py, which this file imports.

THE SCENE is online_checks.scene's construction with its parts kept apart: S = steer * src and N = the white noise, both complex64,
X = complex64(S + N), the z rows of the step-2 form included (Zs, Zn, Z = Zs + Zn: distinct per node and from each other), the same
act[:, 0] = 1 and the same soft masks.

THE REFERENCE is oracle/online_oracle.py:online_mwf's per-frame filter w_all (float64) applied to S and N in float64:
    ref^c[n, t] = sum_p conj(w_all[n, t, p]) V^c[p, n, t].

THE BARS come from the reference side alone, by the protocol of online_checks.py: `online_mwf_f32state_comp` restates the float32-state
recursion with companions (complex64 w, complex64 inputs, complex64 out^c per frame), DIST_REF records per variant and P the worst
per-problem `series` and `frame` distance of that restatement from the float64 reference, separately for `s` and `n` (the noise
companion sits further from the oracle than the mixture does, so the y table is not reused), and a check passes within BAR_FACTOR = 4
times the entry.  tests/test_online_ref_cpu.py recomputes the table and holds the committed figures within [1, 2] x what it finds.
A cut-down run (the emulator) measures the distance on its own inputs, with the same factor.
"""
import zlib

import numpy as np

import online_checks as oc
from oracle import mwf_oracle as mo
from oracle import online_oracle as oo
from oracle import stft_oracle as so

QC = ('series', 'frame')
COMP = ('s', 'n')
E_ARG, E_UNSUPPORTED = -1, -2


# ---- the scene with its parts kept apart ------------------------------------------------------------------------------------------------

def scene_parts(seed, R, K, M, T, step2):
    """online_checks.scene (mask_mode 'soft'), the same draws in the same order -> dict X, S, N (R, K, T, F, M) c64; Z, Zs, Zn
    (R, K, T, F) c64 or None; mask (R, K, T, F) f32.  X = complex64(S + N), Z = complex64(Zs + Zn)."""
    rng = np.random.default_rng(seed)
    F = oc.F_BINS
    C_ = K * M + (K if step2 else 0)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    act = rng.integers(0, 2, (R, T)).astype(np.float64)
    act[:, 0] = 1.0
    steer = cn(R, 1, F, C_)
    src = 2.0 * cn(R, T, F, 1) * act[:, :, None, None]
    s = (steer * src).astype(np.complex64)
    n = cn(R, T, F, C_).astype(np.complex64)
    v = (s + n).astype(np.complex64)
    jit = rng.uniform(-0.05, 0.05, (R, K, T, F))
    mask = np.ascontiguousarray((0.1 + 0.8 * act[:, None, :, None] + jit).astype(np.float32))

    def split(a):
        x = np.ascontiguousarray(a[..., :K * M].reshape(R, T, F, K, M).transpose(0, 3, 1, 2, 4))
        z = np.ascontiguousarray(a[..., K * M:].transpose(0, 3, 1, 2)) if step2 else None
        return x, z
    (X, Z), (S, Zs), (N, Zn) = split(v), split(s), split(n)
    return dict(X=X, Z=Z, S=S, Zs=Zs, N=N, Zn=Zn, mask=mask)


# ---- the float32-state restatement with companions -----------------------------------------------------------------------------------

def online_mwf_f32state_comp(V, mask, comps, lambda_cor=0.95, mu=1.0, update_every=1, init_diag=1e-3):
    """online_checks.online_mwf_f32state carrying companions: the same float32 state and float64 solve, w rounded to complex64, and per
    frame out^c = w^H v^c in complex64 for every V^c (P, n, T) of `comps`.  -> out (n, T), w_last (n, P), [out^c (n, T)] c64."""
    V = np.asarray(V, dtype=np.complex64)
    comps = [np.asarray(c, dtype=np.complex64) for c in comps]
    mask = np.asarray(mask, dtype=np.float32)
    P, n, T = V.shape
    lam = np.float32(lambda_cor)
    oml = np.float32(1.0) - lam
    Rss = np.zeros((n, P, P), np.complex64)
    Rnn = np.tile((np.float32(init_diag) * np.eye(P, dtype=np.float32)).astype(np.complex64), (n, 1, 1))
    w = np.zeros((n, P), np.complex64)
    out = np.zeros((n, T), np.complex64)
    outc = [np.zeros((n, T), np.complex64) for _ in comps]
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
        for o, Vc in zip(outc, comps):
            o[:, t] = np.einsum('np,np->n', np.conjugate(w), np.ascontiguousarray(Vc[:, :, t].T))
            assert o.dtype == np.complex64
    return out, w, outc


def comp_distances(out, ref):
    """Per problem: out (n, T) against the reference -> {'series', 'frame'} of (n,) arrays (online_checks.distances' two output measures)."""
    out = np.asarray(out, np.complex128)
    d = np.abs(out - ref)
    return {'series': np.linalg.norm(out - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300),
            'frame': d.max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)}


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

class RefCase:
    """online_checks.Case with the scene's parts: a variant at one shape; cut = (rooms, frames) takes a prefix."""

    def __init__(self, variant, M, K, cut=None):
        self.variant, self.M, self.K, self.cut = variant, M, K, cut
        self.params, mask_mode, self.T_full = oc.VARIANTS[variant]
        assert mask_mode == 'soft', variant
        self.P = M if K == 1 else M + K - 1
        self.seed = zlib.crc32(f'{variant}/{M}/{K}'.encode())
        self.R, self.T = (oc.R_FULL, self.T_full) if cut is None else (min(cut[0], oc.R_FULL), min(cut[1], self.T_full))
        self._in = self._ref = None

    def inputs(self):
        if self._in is None:
            d = scene_parts(self.seed, oc.R_FULL, self.K, self.M, self.T_full, self.K > 1)
            if self.cut is not None:
                d = {k: None if v is None else np.ascontiguousarray(v[:self.R, :, :self.T]) for k, v in d.items()}
            self._in = d
        return self._in

    def oracle_params(self):
        p = self.params
        return dict(lambda_cor=oc.f32(p['lambda_cor']), mu=oc.f32(p['mu']), update_every=p['update_every'], init_diag=oc.f32(p['init_diag']))

    def problem_rows(self):
        d = self.inputs()
        V, m = oc.problems(d['X'], d['Z'], d['mask'])
        return V, m, oc.problems(d['S'], d['Zs'], d['mask'])[0], oc.problems(d['N'], d['Zn'], d['mask'])[0]

    def reference(self):
        """float64 oracle on every problem: dict out (n, T), w (n, P), w_all (n, T, P), s, n (n, T)."""
        if self._ref is None:
            V, m, VS, VN = self.problem_rows()
            out, w_all = oo.online_mwf(V, m, **self.oracle_params())
            app = lambda Vc: np.einsum('ntp,pnt->nt', np.conjugate(w_all), Vc.astype(np.complex128))
            ref = dict(out=out, w=w_all[:, -1], s=app(VS), n=app(VN))
            for c in COMP:                      # no problem may be skipped: every reference series is non-zero
                assert np.all(np.linalg.norm(ref[c], axis=1) > 0) and np.all(np.linalg.norm(out, axis=1) > 0)
            self._ref = ref
        return self._ref

    def restatement_distance(self):
        """Worst per-problem distance of the float32-state restatement's companions from the reference: {comp: {quantity: float}}."""
        V, m, VS, VN = self.problem_rows()
        _, _, (os_, on_) = online_mwf_f32state_comp(V, m, [VS, VN], **self.oracle_params())
        ref = self.reference()
        return {c: {q: float(v.max()) for q, v in comp_distances(o, ref[c]).items()} for c, o in zip(COMP, (os_, on_))}

    def bar(self):
        """{comp: {quantity: bar}}: the committed table for a full case, measured on the spot for a cut one."""
        if self.cut is None:
            d = {c: dict(zip(QC, DIST_REF[self.variant][self.P][c])) for c in COMP}
        else:
            d = self.restatement_distance()
        return {c: {q: oc.BAR_FACTOR * d[c][q] for q in QC} for c in COMP}


_cases = {}


def case(variant, M, K, cut=None):
    key = (variant, M, K, cut)
    if key not in _cases:
        _cases[key] = RefCase(variant, M, K, cut)
    return _cases[key]


def table_cases():
    """Every full case the checks take a bar from: variant -> list of (M, K)."""
    main = [(P, 1) for P in oc.STEP1_SIZES] + list(oc.STEP2_SHAPES)
    t = {'d1': main, 'd1e-3': main}
    for v in oc.SCHEDULES:
        t[v] = [(P, 1) for P in oc.SCHEDULE_SIZES]
    return t


def recompute_dist(variants=None, verbose=False):
    """DIST_REF from scratch: variant -> {P: {'s': (series, frame), 'n': (series, frame)}}, the worst over the cases at that P."""
    res = {}
    for v, shapes in table_cases().items():
        if variants is not None and v not in variants:
            continue
        res[v] = {}
        for M, K in shapes:
            c = RefCase(v, M, K)
            d = c.restatement_distance()
            old = res[v].get(c.P, {k: (0.0, 0.0) for k in COMP})
            res[v][c.P] = {k: tuple(max(o, d[k][q]) for o, q in zip(old[k], QC)) for k in COMP}
            if verbose:
                print(v, (M, K), c.P, d, flush=True)
    return res


def print_dist():
    t = recompute_dist(verbose=True)
    print('DIST_REF = {')
    for v, rows in t.items():
        print(f'    {v!r}: {{')
        for P in sorted(rows):
            print(f'        {P}: {{' + ', '.join(f"'{k}': ({', '.join(f'{oc.round_up(x):.1e}' for x in rows[P][k])})" for k in COMP) + '},')
        print('    },')
    print('}')


# Worst per-problem distance between online_mwf_f32state_comp's companions and the float64 reference:
# variant -> {P: {'s': (series, frame), 'n': (series, frame)}}.  Written by
#   python -c "import online_ref_checks as rc; rc.print_dist()"       (in tests/)
# (what the recomputation printed, times 1.1, rounded up to two digits) and checked against a recomputation by
# tests/test_online_ref_cpu.py.  The bar of a check is BAR_FACTOR times its entry.
DIST_REF = {
    'd1': {
        1: {'s': (2.0e-07, 2.6e-07), 'n': (2.1e-07, 3.3e-07)},
        2: {'s': (6.4e-07, 9.0e-07), 'n': (6.2e-07, 9.2e-07)},
        3: {'s': (6.0e-07, 9.8e-07), 'n': (4.4e-07, 6.0e-07)},
        4: {'s': (4.4e-07, 5.2e-07), 'n': (5.3e-07, 1.1e-06)},
        5: {'s': (3.8e-07, 4.7e-07), 'n': (6.2e-07, 1.4e-06)},
        6: {'s': (2.5e-07, 2.8e-07), 'n': (4.4e-07, 7.2e-07)},
        7: {'s': (3.3e-07, 4.1e-07), 'n': (5.0e-07, 7.7e-07)},
        8: {'s': (8.1e-07, 9.4e-07), 'n': (5.7e-07, 8.0e-07)},
        9: {'s': (1.7e-07, 2.4e-07), 'n': (6.4e-07, 9.5e-07)},
        10: {'s': (1.8e-07, 2.4e-07), 'n': (4.2e-07, 6.2e-07)},
        11: {'s': (2.3e-07, 3.3e-07), 'n': (5.3e-07, 9.8e-07)},
        12: {'s': (3.7e-07, 4.2e-07), 'n': (5.5e-07, 1.1e-06)},
        13: {'s': (1.7e-07, 2.6e-07), 'n': (8.1e-07, 1.5e-06)},
        14: {'s': (2.0e-07, 2.7e-07), 'n': (7.3e-07, 9.9e-07)},
        15: {'s': (2.0e-07, 2.9e-07), 'n': (7.8e-07, 1.4e-06)},
        16: {'s': (2.4e-07, 3.3e-07), 'n': (9.0e-07, 1.6e-06)},
    },
    'd1e-3': {
        1: {'s': (1.5e-07, 1.9e-07), 'n': (1.1e-07, 1.6e-07)},
        2: {'s': (2.6e-05, 4.1e-05), 'n': (2.9e-05, 3.8e-05)},
        3: {'s': (1.3e-05, 1.6e-05), 'n': (2.0e-05, 3.2e-05)},
        4: {'s': (2.5e-05, 3.6e-05), 'n': (3.8e-05, 5.5e-05)},
        5: {'s': (4.4e-05, 6.8e-05), 'n': (1.4e-04, 2.7e-04)},
        6: {'s': (3.6e-05, 5.3e-05), 'n': (6.5e-05, 1.3e-04)},
        7: {'s': (5.7e-05, 7.1e-05), 'n': (8.4e-05, 1.2e-04)},
        8: {'s': (8.5e-05, 1.2e-04), 'n': (1.1e-04, 1.3e-04)},
        9: {'s': (9.6e-05, 1.8e-04), 'n': (2.9e-04, 4.8e-04)},
        10: {'s': (4.8e-05, 8.2e-05), 'n': (1.6e-04, 2.2e-04)},
        11: {'s': (8.6e-05, 1.1e-04), 'n': (3.1e-04, 5.4e-04)},
        12: {'s': (8.9e-05, 1.2e-04), 'n': (2.1e-04, 3.0e-04)},
        13: {'s': (1.6e-04, 1.9e-04), 'n': (3.0e-04, 4.2e-04)},
        14: {'s': (9.6e-05, 1.7e-04), 'n': (2.1e-04, 3.3e-04)},
        15: {'s': (2.1e-04, 2.7e-04), 'n': (3.2e-04, 6.0e-04)},
        16: {'s': (3.1e-04, 4.8e-04), 'n': (4.0e-04, 6.6e-04)},
    },
    'u1': {
        3: {'s': (2.1e-07, 2.2e-07), 'n': (3.3e-07, 5.7e-07)},
        8: {'s': (1.4e-07, 1.9e-07), 'n': (3.6e-07, 5.0e-07)},
        13: {'s': (1.7e-07, 2.3e-07), 'n': (4.9e-07, 7.5e-07)},
    },
    'u2': {
        3: {'s': (4.6e-07, 4.9e-07), 'n': (6.2e-07, 5.1e-07)},
        8: {'s': (1.7e-07, 2.2e-07), 'n': (3.2e-07, 5.2e-07)},
        13: {'s': (1.9e-07, 2.7e-07), 'n': (3.5e-07, 5.2e-07)},
    },
    'u3': {
        3: {'s': (1.3e-06, 1.5e-06), 'n': (5.7e-07, 8.2e-07)},
        8: {'s': (2.0e-07, 2.2e-07), 'n': (3.5e-07, 4.7e-07)},
        13: {'s': (1.5e-07, 2.8e-07), 'n': (4.8e-07, 6.6e-07)},
    },
    'uTm1': {
        3: {'s': (4.1e-07, 5.5e-07), 'n': (4.4e-07, 6.0e-07)},
        8: {'s': (3.8e-07, 4.1e-07), 'n': (5.0e-07, 6.8e-07)},
        13: {'s': (1.6e-07, 2.2e-07), 'n': (3.6e-07, 5.1e-07)},
    },
    'uT': {
        3: {'s': (2.1e-06, 2.8e-06), 'n': (1.5e-07, 1.8e-07)},
        8: {'s': (1.7e-07, 2.3e-07), 'n': (1.7e-07, 2.6e-07)},
        13: {'s': (1.8e-07, 2.1e-07), 'n': (1.8e-07, 2.4e-07)},
    },
    'uTp5': {
        3: {'s': (3.4e-07, 3.6e-07), 'n': (1.7e-07, 2.4e-07)},
        8: {'s': (6.6e-07, 7.3e-07), 'n': (1.6e-07, 2.2e-07)},
        13: {'s': (2.4e-07, 2.6e-07), 'n': (1.8e-07, 2.4e-07)},
    },
}


# ---- driving the kernels ------------------------------------------------------------------------------------------------------------------

def _flat(buf, T):
    a = buf.numpy()
    return np.ascontiguousarray(a.transpose(0, 1, 3, 2)).reshape(-1, T)


def run_ref(make_engine, d, K, params, options=None, shard=None, zblk=None, n_comp=2, plain=False):
    """Engine.online_mwf_ref on the scene d -> dict out, s[, n] (n_prob, T), w (n_prob, P) in problem order (room, node, bin).
    plain=True: Engine.online_mwf on the same engine state instead (out, w).  shard / zblk as online_checks.run_kernel."""
    X, mask = d['X'], d['mask']
    R, _, T, F, M = X.shape
    eng = make_engine(rooms=R, nodes=K, mics=M, length=(T - 1) * oc.HOP, n_fft=oc.N_FFT)
    assert (eng.T, eng.F) == (T, F), (eng.T, eng.F)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    S, N = d['S'], d['N']
    if shard is not None:
        k0, Kl = shard
        eng.set_node_shard(k0, Kl)
        X, mask, S, N = (np.ascontiguousarray(a[:, k0:k0 + Kl]) for a in (X, mask, S, N))
    Z, Zs, Zn = d['Z'], d['Zs'], d['Zn']
    if zblk is not None:
        eng.set_z_blocks(zblk)
        Z, Zs, Zn = (oc.z_blocks(a, zblk) for a in (Z, Zs, Zn))
    if plain:
        out, w = eng.online_mwf(X, mask, Z=Z, want_w=True, **params)
        res = dict(out=_flat(out, T), w=w.numpy().reshape(-1, w.shape[-1]))
    else:
        r = eng.online_mwf_ref(X, mask, S, N if n_comp == 2 else None, Z=Z, Zs=Zs, Zn=Zn if n_comp == 2 else None, want_w=True, **params)
        res = dict(out=_flat(r[0], T), s=_flat(r[1], T), w=r[-1].numpy().reshape(-1, r[-1].shape[-1]))
        if n_comp == 2:
            res['n'] = _flat(r[2], T)
    eng.close()
    return res


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def compare_case(make_engine, c, route_list=None, seen=None, **run):
    """Case c on every route (or those named): companions against the reference inside their bars (check 1), out and w_last
    np.array_equal to the plain call's on the same inputs, route and options (check 2)."""
    d, ref, bar = c.inputs(), c.reference(), c.bar()
    sel = slice(None)
    if run.get('shard') is not None:
        k0, Kl = run['shard']
        n1 = oc.F_BINS
        sel = np.concatenate([np.arange((r * c.K + k) * n1, (r * c.K + k + 1) * n1) for r in range(c.R) for k in range(k0, k0 + Kl)])
    for name, opts in oc.routes(c.P):
        if route_list is not None and name not in route_list:
            continue
        got = run_ref(make_engine, d, c.K, c.params, options=opts, **run)
        plain = run_ref(make_engine, d, c.K, c.params, options=opts, plain=True, **run)
        assert np.array_equal(got['out'], plain['out']) and np.array_equal(got['w'], plain['w']), (c.variant, c.M, c.K, name, 'mixture branch moved')
        line = []
        for k in COMP:
            assert np.isfinite(got[k].view(np.float32)).all(), (c.variant, c.M, c.K, name, k)
            dist = comp_distances(got[k], ref[k][sel])
            for q in QC:
                i = int(np.argmax(dist[q]))
                worst = float(dist[q][i])
                line.append(f'{k}.{q}={worst:.2e}/{bar[k][q]:.2e}')
                if seen is not None:
                    cur = seen.setdefault(c.P, {}).setdefault(name, {})
                    cur[f'{k}.{q}'] = max(cur.get(f'{k}.{q}', 0.0), worst)
        print(f'online_ref {c.variant} M={c.M} K={c.K} P={c.P} {name} {run if run else ""}: ' + ' '.join(line), flush=True)
        for k in COMP:
            dist = comp_distances(got[k], ref[k][sel])
            for q in QC:
                i = int(np.argmax(dist[q]))
                assert dist[q][i] <= bar[k][q], ((c.variant, c.M, c.K, name, run), k, q, 'problem', i, float(dist[q][i]), 'bar', bar[k][q])


# ---- checks 1 + 2: every size and route; the mixture branch untouched -----------------------------------------------------------------

def check_sizes(make_engine, variant='d1', step1=oc.STEP1_SIZES, step2=oc.STEP2_SHAPES, cut=None):
    seen = {}
    for M, K in [(P, 1) for P in step1] + list(step2):
        compare_case(make_engine, case(variant, M, K, cut), seen=seen)
    return seen


# ---- check 3: the filter in force -----------------------------------------------------------------------------------------------------

def check_schedule(make_engine, sizes=oc.SCHEDULE_SIZES, cut=None):
    """update_every over online_checks.SCHEDULES: the `frame` quantity compares frame by frame, so a companion filtered with the next
    or the previous update's filter fails it."""
    seen = {}
    for name in oc.SCHEDULES:
        for P in sizes:
            compare_case(make_engine, RefCase(name, P, 1, cut), route_list=('thread', 'group'), seen=seen.setdefault(name, {}))
    return seen


# ---- check 4: row order and layouts ----------------------------------------------------------------------------------------------------

def check_row_order(make_engine, shapes=((2, 6, 3), (8, 9, 3)), variant='d1', cut=None, every_k0=True):
    """Node shards at every k0 against the reference rows (Zs, Zn, Z distinct per node and from each other: a companion that reads Z for
    Zs fails); rank-major z blocks bit-identical to the plain layout in all four outputs."""
    seen = {}
    for M, K, blk in shapes:
        c = case(variant, M, K, cut)
        d = c.inputs()
        assert not np.array_equal(d['Zs'], d['Z']) and not np.array_equal(d['Zn'], d['Z']) and not np.array_equal(d['Zs'], d['Zn'])
        assert len({d['Zs'][0, j, 0, 5] for j in range(K)}) == K and len({d['Zn'][0, j, 0, 5] for j in range(K)}) == K     # (frame 0: the source is on)
        rl = ('thread', 'group')
        for shard in [(k0, 1) for k0 in (range(K) if every_k0 else (0, K // 2, K - 1))] + [(K // 2 - 1, 2)]:
            compare_case(make_engine, c, route_list=rl, seen=seen, shard=shard)
        for name, opts in oc.routes(c.P):
            if name not in rl:
                continue
            for shard in (None, (K // 2 - 1, 2)):
                plain = run_ref(make_engine, d, K, c.params, options=opts, shard=shard)
                for b in sorted({blk, K // blk}):
                    blocked = run_ref(make_engine, d, K, c.params, options=opts, shard=shard, zblk=b)
                    for key in ('out', 's', 'n', 'w'):
                        assert same(plain[key], blocked[key]), (M, K, name, shard, b, key)
    return seen


# ---- check 5: one companion --------------------------------------------------------------------------------------------------------------

def check_one_companion(make_engine, shapes=((3, 1), (6, 1), (2, 6), (8, 9)), variant='d1', cut=None):
    for M, K in shapes:
        c = case(variant, M, K, cut)
        for name, opts in oc.routes(c.P):
            if name == 'thread_sq64':
                continue
            two = run_ref(make_engine, c.inputs(), K, c.params, options=opts)
            one = run_ref(make_engine, c.inputs(), K, c.params, options=opts, n_comp=1)
            assert 'n' not in one
            for key in ('out', 's', 'w'):
                assert same(two[key], one[key]), (M, K, name, key)


# ---- check 6: containment ----------------------------------------------------------------------------------------------------------------

def check_containment(make_engine, step1=(4, 7, 8, 16), step2=((2, 3), (2, 6), (8, 9)), variant='d1', cut=None):
    """One NaN in S at one (problem, frame): out_s non-finite at that problem and frame only; every other out_s value, all of out_n, out
    and w_last bit-identical to the clean run (companions do not feed the recursion).  Then a NaN in one remote Zs row."""
    F = oc.F_BINS
    for M, K in [(P, 1) for P in step1] + list(step2):
        c = case(variant, M, K, cut)
        d = c.inputs()
        t0, r, k, f = c.T // 2, c.R - 1, K // 2, 77
        for name, opts in oc.routes(c.P):
            if name == 'thread_sq64':
                continue
            clean = run_ref(make_engine, d, K, c.params, options=opts)
            bad = dict(d, S=d['S'].copy())
            bad['S'][r, k, t0, f, M - 1] = np.nan
            got = run_ref(make_engine, bad, K, c.params, options=opts)
            hit = np.zeros(clean['s'].shape, bool)
            hit[(r * K + k) * F + f, t0] = True
            _contained(got, clean, hit, (M, K, name, 'NaN in S'))
            if K == 1:
                continue
            j = (k + 1) % K                                              # a remote row of every node but j
            bad = dict(d, Zs=d['Zs'].copy())
            bad['Zs'][r, j, t0, f] = np.nan
            got = run_ref(make_engine, bad, K, c.params, options=opts)
            hit = np.zeros(clean['s'].shape, bool)
            for kk in range(K):
                if kk != j:
                    hit[(r * K + kk) * F + f, t0] = True
            _contained(got, clean, hit, (M, K, name, 'NaN in a remote Zs row'))


def _contained(got, clean, hit, what):
    assert not np.isfinite(got['s'][hit]).any(), (what, 'a poisoned value came out finite')
    assert same(got['s'][~hit], clean['s'][~hit]), (what, 'other out_s values moved')
    for key in ('n', 'out', 'w'):
        assert same(got[key], clean[key]), (what, key, 'moved')


# ---- check 7: refusals ---------------------------------------------------------------------------------------------------------------------

def check_refusals(make_engine):
    """Every refusal returns its documented code and leaves sentinel-filled out, out_s, out_n untouched (the C ABI directly)."""
    from disco_amd import _lib as L
    T = 4
    sent = 7.0 - 3.0j

    def call(eng, P, with_z=True, lam=0.95, U=1, init=1e-3, n_comp=2, drop=None):
        R, K, M, F = eng.R, eng.K, eng.M, eng.F
        rng = np.random.default_rng(5)
        cx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(np.complex64)
        keep = []

        def dev(a, dt):
            p, k_ = eng.to_device(a, dt)
            keep.append(k_)
            return p
        px, pm = dev(cx(R, K, T, F, M), np.complex64), dev(np.full((R, K, T, F), 0.5, np.float32), np.float32)
        pz = dev(cx(R, K, T, F), np.complex64) if with_z else None
        outs = [eng.to_device(np.full((R, K, T, F), sent, np.complex64), np.complex64)[1] for _ in range(3)]
        comp = (L.DiscoOnlineCompanion * 2)()
        for i in range(2):
            comp[i].X, comp[i].Z, comp[i].out = dev(cx(R, K, T, F, M), np.complex64), dev(cx(R, K, T, F), np.complex64), outs[1 + i].ptr
        if drop == 'X':
            comp[1].X = None
        elif drop == 'out':
            comp[0].out = None
        elif drop == 'Z':
            comp[1].Z = None
        elif drop == 'comp':
            comp = None
        rc = eng.lib.disco_online_mwf_ref(eng.ctx, px, pz, pm, P, lam, 1.0, U, init, outs[0].ptr, None, comp, n_comp, eng.stream)
        eng.sync()
        return rc, all(np.all(o.numpy() == np.complex64(sent)) for o in outs), eng.lib.disco_last_error(eng.ctx).decode()
    eng = make_engine(rooms=1, nodes=3, mics=2, length=(T - 1) * oc.HOP, n_fft=oc.N_FFT)
    rc, untouched, _ = call(eng, 4)
    assert rc == 0 and not untouched                                      # the harness itself: a good call writes
    rc, untouched, _ = call(eng, 2, drop='Z')
    assert rc == 0 and not untouched                                      # P = mics: a companion's Z is not needed
    for what, kw, want in (('lambda = 1', dict(P=4, lam=1.0), E_ARG), ('lambda NaN', dict(P=4, lam=float('nan')), E_ARG),
                           ('update_every = 0', dict(P=4, U=0), E_ARG), ('init_diag = 0', dict(P=4, init=0.0), E_ARG),
                           ('P = 3', dict(P=3), E_ARG), ('P > M without Z', dict(P=4, with_z=False), E_ARG),
                           ('n_comp = 0', dict(P=4, n_comp=0), E_ARG), ('n_comp = 3', dict(P=4, n_comp=3), E_ARG),
                           ('no companions', dict(P=4, drop='comp'), E_ARG), ('companion without X', dict(P=4, drop='X'), E_ARG),
                           ('companion without out', dict(P=4, drop='out'), E_ARG), ('P > M, companion without Z', dict(P=4, drop='Z'), E_ARG)):
        rc, untouched, msg = call(eng, **kw)
        assert rc == want and untouched and 'disco_online_mwf_ref' in msg, (what, rc, untouched, msg)
    eng.set_lengths([2 * oc.HOP])
    rc, untouched, msg = call(eng, 4)
    assert rc == E_UNSUPPORTED and untouched and 'lengths' in msg, (rc, untouched, msg)
    eng.close()
    eng = make_engine(rooms=1, nodes=10, mics=8, length=(T - 1) * oc.HOP, n_fft=oc.N_FFT)          # P2 = 17
    rc, untouched, msg = call(eng, 17)
    assert rc == E_UNSUPPORTED and untouched and '16' in msg, (rc, untouched, msg)
    eng.close()
    # the whole-path call: lengths set, a shard active, P2 = 17 -- nothing written
    for setup, K, M in ((lambda e: e.set_lengths([2 * oc.HOP]), 3, 2), (lambda e: e.set_node_shard(1, 2), 3, 2),
                        (lambda e: e.set_z_blocks(1), 3, 2), (lambda e: None, 10, 8)):
        eng = make_engine(rooms=1, nodes=K, mics=M, length=(T - 1) * oc.HOP, n_fft=oc.N_FFT)
        setup(eng)
        y = np.random.default_rng(3).standard_normal((3, 1, K, M, eng.Lsamp)).astype(np.float32)
        dev = [eng.to_device(a, np.float32) for a in y]
        bufs = {nm: eng.to_device(np.full((1, K, eng.T, eng.F), 7.0, np.float32 if nm.startswith('mask') else np.complex64),
                                  np.float32 if nm.startswith('mask') else np.complex64)[1]
                for nm in ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w')}
        sig = eng.to_device(np.full((6, 1, K, eng.Lsamp), 7.0, np.float32), np.float32)[1]
        outs = L.DiscoRefOutputs(**{nm: b.ptr for nm, b in bufs.items()})
        import ctypes as C
        rc = eng.lib.disco_tango_online_reference(eng.ctx, dev[0][0], dev[1][0], dev[2][0], None, None, 0.95, 1, 1e-3, C.byref(outs), sig.ptr,
                                                  None, 0, eng.stream)
        eng.sync()
        msg = eng.lib.disco_last_error(eng.ctx).decode()
        assert rc == E_UNSUPPORTED and 'disco_tango_online_reference' in msg, (K, M, rc, msg)
        assert all(np.all(b.numpy() == 7.0) for b in bufs.values()) and np.all(sig.numpy() == 7.0), (K, M, 'a refused call wrote')
        eng.close()


# ---- check 8: the whole path ---------------------------------------------------------------------------------------------------------------

def online_tango_ref64(y, s, n, n_fft=512, update_every=1, lambda_cor=0.95, mu=1.0, init_diag=1e-3):
    """oracle/online_oracle.py:online_tango of one room with the images carried along: the filters of every frame (online_mwf's w_all,
    float64) applied to S and N; the exchanged rows rounded to complex64 as online_tango rounds z.  -> dict z_y, z_s, z_n, yf, sf, nf
    (K, F, T) c128."""
    K, M, L = y.shape
    hop = n_fft // 2
    tr = lambda a: np.stack([np.stack([so.stft(a[k, m], n_fft, hop, 'reflect') for m in range(M)]) for k in range(K)])
    Y, S, N = tr(y), tr(s), tr(n)
    masks = np.stack([mo.tf_mask(S[k, 0], N[k, 0], 'irm1') for k in range(K)])
    app = lambda w_all, V: np.einsum('ftp,pft->ft', np.conjugate(w_all), V.astype(np.complex128))
    z = {c: [] for c in 'ysn'}
    for k in range(K):
        out, w_all = oo.online_mwf(Y[k], masks[k], lambda_cor, mu, update_every, init_diag)
        z['y'].append(out), z['s'].append(app(w_all, S[k])), z['n'].append(app(w_all, N[k]))
    z = {c: np.stack(v) for c, v in z.items()}
    z32 = {c: v.astype(np.complex64) for c, v in z.items()}
    f = {c: [] for c in 'ysn'}
    rows = lambda A, zz, k: np.concatenate([A[k]] + [zz[j][None] for j in range(K) if j < k] + [zz[j][None] for j in range(K) if j > k], 0)
    for k in range(K):
        out, w_all = oo.online_mwf(rows(Y, z32['y'], k), masks[k], lambda_cor, mu, update_every, init_diag)
        f['y'].append(out), f['s'].append(app(w_all, rows(S, z32['s'], k))), f['n'].append(app(w_all, rows(N, z32['n'], k)))
    return dict(z_y=z['y'], z_s=z['s'], z_n=z['n'], yf=np.stack(f['y']), sf=np.stack(f['s']), nf=np.stack(f['n']))


def check_whole_path(make_engine, R=2, K=3, M=2, L=6000, update_every=1, tol=1e-4, options=None):
    """tango_online_reference on check_online_mwf's rooms (parity_checks: disco_amd.synth, tol = 1e-4 with its relative-error measure)."""
    from disco_amd import synth
    import parity_checks as pc
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    T, F = eng.T, eng.F
    d = eng.tango_online_reference(y, s, n, update_every=update_every, signals=True)
    sig = d.pop('signals').numpy()
    h = {k: v.numpy() for k, v in d.items()}
    # the oracle masks are tango_reference's, bit for bit
    ref = eng.tango_reference(y, s, n, want=('masks_z', 'mask_w'))
    assert same(h['masks_z'], ref['masks_z'].numpy()) and same(h['mask_w'], ref['mask_w'].numpy())
    # the mixture branch is tango_online's with the same masks, bit for bit
    out, z, yf = eng.tango_online(y, h['masks_z'], h['mask_w'], update_every=update_every)
    assert same(h['z_y'], z.numpy()) and same(h['yf'], yf.numpy()) and same(sig[0], out.numpy())
    # zn = Y[ref] - z_y against disco_noise_residual
    X = eng.stft(y.reshape(R * K, M, L)).reshape(R, K, T, F, M)
    assert same(h['zn'], eng.noise_residual(X, d['z_y']).numpy())
    # the six time signals are the inverse transforms of the six spectra.  The online entry points invert ONE frame per transform
    # (k_istft<N, SOLO>: what lets the stream equal the whole clip bit for bit) while Engine.istft packs two frames into one complex
    # transform, so the two are two float32 roundings of one inverse transform and cannot agree to the bit while signal 0 equals
    # tango_online's out to the bit (asserted above).  The bound: log2(n_fft) butterfly stages of one rounding each, two inversions, two
    # overlapped frames per sample -> 4 log2(n_fft) eps32 of the signal's peak (the packed partner's magnitude enters a frame's rounding).
    bound = 4 * np.log2(eng.n_fft) * float(np.finfo(np.float32).eps)
    for i, nm in enumerate(('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n')):
        inv = eng.istft(d[nm].reshape(R * K, T, F)).numpy()
        dev = float(np.abs(sig[i].reshape(R * K, L) - inv).max() / np.abs(inv).max())
        print(f'online_ref signal {nm}: max |solo - paired inverse| / peak = {dev:.2e} (bound {bound:.2e})', flush=True)
        assert dev <= bound, (nm, dev, bound)
    # the companions against the float64 restatement
    errs = {}
    for r in range(R):
        o = online_tango_ref64(y[r], s[r], n[r], update_every=update_every)
        for nm in ('z_s', 'z_n', 'sf', 'nf', 'z_y', 'yf'):
            for k in range(K):
                errs[nm] = max(errs.get(nm, 0.0), pc.relerr(h[nm][r, k].T, o[nm][k]))
    print('online_ref whole path', (R, K, M, L), {k: f'{v:.2e}' for k, v in errs.items()}, 'tol', tol, flush=True)
    assert all(v < tol for v in errs.values()), errs
    eng.close()
    return errs


# ---- check 9: the surface ---------------------------------------------------------------------------------------------------------------------

def check_surface(R=2, K=3, M=2, L=6000):
    """online_tango_batched / online_tango (disco_amd.speech_enhancement.tango) on the library the package loads."""
    from disco_amd import synth
    from disco_amd.speech_enhancement import tango
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    off = tango.offline_tango_batched(y, s, n)
    on = tango.online_tango_batched(y, s, n)
    assert list(on) == list(off)
    for nm in off:
        assert on[nm].shape == off[nm].shape and on[nm].dtype == off[nm].dtype, (nm, on[nm].shape, on[nm].dtype)
    assert same(on['masks_z'], off['masks_z']) and same(on['mask_w'], off['mask_w'])
    one = tango.online_tango(y[0], s[0], n[0])
    ref = tango.offline_tango(y[0], s[0], n[0])
    names = ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w')
    row0 = tango.online_tango_batched(y[:1], s[:1], n[:1])
    for i, nm in enumerate(names):
        assert len(one[i]) == K and one[i][0].shape == ref[i][0].shape
        for k in range(K):
            assert same(one[i][k], np.ascontiguousarray(row0[nm][0, k].T)), (nm, k)
            assert same(one[i][k], np.ascontiguousarray(on[nm][0, k].T)), (nm, k, 'a room depends on its batch')
    # masks= overrides vads
    mz = np.clip(on['masks_z'] * 0.5 + 0.1, 0, 1).astype(np.float32)
    a = tango.online_tango_batched(y, s, n, vads='ivad', masks=(mz, None))
    b = tango.online_tango_batched(y, s, n, vads='irm1', masks=(mz, mz))
    assert same(a['masks_z'], mz) and same(a['mask_w'], mz) and not same(a['yf'], on['yf'])
    for nm in names:
        assert same(a[nm], b[nm]), nm
    for bad in ('ivad', 'crnn', 'rnn', 'nonsense'):
        try:
            tango.online_tango_batched(y, s, n, vads=bad)
        except NotImplementedError as e:
            assert 'masks=' in str(e), e
        else:
            raise AssertionError(f'vads={bad!r} was accepted')
    return on
