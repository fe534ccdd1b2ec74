"""The reference side of the online-size checks (tests/online_checks.py), no GPU and no kernel: the float32-state restatement of the
oracle is the oracle's recursion (the reference's own outputs, tests/golden/online_ref.npz), the committed table of its distance from
the float64 oracle is what a recomputation finds (not smaller: the reference alone stays inside every bar; not more than twice as
large: the bars do not quietly loosen), and the helpers that lay inputs out for the kernel say what include/disco_hip.h says."""
import os

import numpy as np
import pytest

import online_checks as oc
from oracle import online_oracle as oo


@pytest.mark.parametrize('variant', sorted(oc.table_cases()))
def test_committed_distances_match_recomputation(variant):
    found = oc.recompute_dist(variants=(variant,))[variant]
    assert sorted(found) == sorted(oc.DIST[variant]), (sorted(found), sorted(oc.DIST[variant]))
    for P, row in found.items():
        for q, got, committed in zip(oc.QUANT, row, oc.DIST[variant][P]):
            print(variant, P, q, f'{got:.3e}', f'{committed:.3e}')
            assert got <= committed <= 2.0 * got, (variant, P, q, got, committed)


def test_table_covers_every_size_and_route():
    for v in ('d1', 'd1e-3'):
        assert sorted(oc.DIST[v]) == list(range(1, 17))
    assert {M + K - 1 for M, K in oc.STEP2_SHAPES} == set(range(2, 17))
    assert (8, 9) in oc.STEP2_SHAPES and (1, 16) in oc.STEP2_SHAPES and any(K >= 6 for _, K in oc.STEP2_SHAPES)
    for P in range(1, 17):
        names = [n for n, _ in oc.routes(P)]
        assert names == (['thread', 'thread_sq64'] if P <= 4 else ['thread', 'thread_sq64', 'group'] if P <= 7 else ['group'])
    assert dict(oc.routes(6))['group'] == {'solve_thread': 0} and dict(oc.routes(6))['thread']['solve_thread'] == 1
    # the step-1 form of every P (and the one-room cut) leaves the last block of 16 (8 lanes) / 4 (16 lanes) problems partly dead
    assert (oc.R_FULL * oc.F_BINS) % 16 and (oc.R_FULL * oc.F_BINS) % 4 and oc.F_BINS % 16 and oc.F_BINS % 4
    assert max(abs(np.log10(x * 1.1 / oc.round_up(x))) for x in (1.234e-7, 9.99e-5, 1.0e-6)) < 0.05
    assert all(oc.round_up(x) >= 1.1 * x * (1 - 1e-12) for x in (1.234e-7, 9.99e-5, 1.0e-6, 3.3e-7))


def test_restatement_is_the_pinned_recursion(golden_dir):
    """On the inputs of the reference's own run: the restatement's state is float32 (asserted inside it), its outputs sit at float32
    distance from the reference's -- the existing bar of check_online_golden, 5e-5 -- and not at float64 distance (it does round)."""
    g = np.load(os.path.join(golden_dir, 'online_ref.npz'))
    for tag in ('p3', 'p5u4'):
        V, mask, ref, w_ref = g[tag + '_V'], g[tag + '_mask'], g[tag + '_out'], g[tag + '_w']
        lam, mu, init, U = (float(x) for x in g[tag + '_params'])
        out, w = oc.online_mwf_f32state(V, mask, lam, mu, int(U), init)
        assert out.dtype == np.complex64 and w.dtype == np.complex64
        d = oc.distances(out, w, ref, w_ref[:, -1])
        print(tag, {q: float(d[q].max()) for q in oc.QUANT})
        assert all(1e-9 < float(d[q].max()) < 5e-5 for q in oc.QUANT), {q: float(d[q].max()) for q in oc.QUANT}
        o64, w64 = oo.online_mwf(V, mask, lam, mu, int(U), init)
        assert np.abs(o64 - ref).max() < 1e-9 * np.abs(ref).max()


def test_problem_rows_follow_the_reference_order():
    """[Y_k ; z_j, j < k ; z_j, j > k] (tango.py:142-155), problems in (room, node, bin) order, z distinct per node."""
    X, Z, mask = oc.scene(3, 2, 4, 2, 3, True)
    R, K, T, F, M = X.shape
    assert Z.shape == (R, K, T, F) and mask.shape == (R, K, T, F) and mask.dtype == np.float32 and X.dtype == np.complex64
    assert len({Z[1, j, 2, 5] for j in range(K)}) == K
    V, m = oc.problems(X, Z, mask)
    assert V.shape == (M + K - 1, R * K * F, T) and m.shape == (R * K * F, T)
    r, k, f, t = 1, 2, 100, 1
    pid = (r * K + k) * F + f
    want = [X[r, k, t, f, 0], X[r, k, t, f, 1], Z[r, 0, t, f], Z[r, 1, t, f], Z[r, 3, t, f]]
    assert np.array_equal(V[:, pid, t], np.array(want)) and m[pid, t] == mask[r, k, t, f]
    V1, _ = oc.problems(X, Z, mask, nodes=[2])
    assert np.array_equal(V1[:, 1 * F + f, t], np.array(want))
    # the same rows as oracle/online_oracle.py:online_tango concatenates for its step 2
    Y = X[r].transpose(0, 3, 2, 1)                                       # (K, M, F, T)
    z32 = Z[r].transpose(0, 2, 1)                                        # (K, F, T)
    rows = [Y[k]] + [z32[j][None] for j in range(K) if j < k] + [z32[j][None] for j in range(K) if j > k]
    assert np.array_equal(np.concatenate(rows, 0), V[:, (r * K + k) * F:(r * K + k + 1) * F])


def test_scene_masks_and_prefix():
    """Mask modes are what the edge checks say they are; a cut case is the prefix of the full one."""
    for mode, vals in (('binary', {0.0, 1.0}), ('ones', {1.0}), ('zeros', {0.0})):
        assert set(np.unique(oc.scene(9, 2, 1, 3, 6, False, mode)[2]).tolist()) == vals
    soft = oc.scene(9, 2, 1, 3, 6, False)[2]
    assert 0.04 < soft.min() < 0.16 and 0.84 < soft.max() < 0.96
    full, cut = oc.Case('d1', 2, 3), oc.Case('d1', 2, 3, cut=(1, 5))
    for a, b in zip(full.inputs(), cut.inputs()):
        assert np.array_equal(a[:1, :, :5], b)
    assert (cut.R, cut.T, cut.P) == (1, 5, 4)


def test_z_block_layout_is_the_documented_one():
    """disco_set_z_blocks: planes [K / blk][R][blk] (csrc/common.h z_plane)."""
    R, K, blk = 3, 6, 2
    Z = np.arange(R * K * 5, dtype=np.float64).reshape(R, K, 5).astype(np.complex64)
    B = oc.z_blocks(Z, blk).reshape(-1, 5)
    for r in range(R):
        for j in range(K):
            assert np.array_equal(B[((j // blk) * R + r) * blk + j % blk], Z[r, j])


def test_schedule_cases_pin_the_first_solve():
    """update_every >= T: the oracle's filter never changes after frame 0, and frame 0's Rnn is lambda init_diag I + one outer product."""
    for name in ('uT', 'uTp5'):
        c = oc.Case(name, 3, 1, cut=(1, oc.T_SCHED))
        V, m = oc.problems(*c.inputs())
        w_all = oo.online_mwf(V, m, **c.oracle_params())[1]
        assert np.array_equal(w_all[:, -1], w_all[:, 0]) and np.abs(w_all[:, 0]).min() > 0
    c = oc.Case('uTm1', 3, 1, cut=(1, oc.T_SCHED))
    V, m = oc.problems(*c.inputs())
    w_all = oo.online_mwf(V, m, **c.oracle_params())[1]
    assert np.array_equal(w_all[:, -2], w_all[:, 0]) and not np.array_equal(w_all[:, -1], w_all[:, 0])
