"""The reference side of the companion checks (tests/online_ref_checks.py), no GPU and no kernel: the committed table DIST_REF is what
a recomputation finds (not smaller: the reference side alone stays inside every bar; not more than twice as large: the bars do not
quietly loosen), the scene's parts add up to the scene, and the restatement with companions is online_checks' restatement."""
import numpy as np
import pytest

import online_checks as oc
import online_ref_checks as rc
from oracle import online_oracle as oo


@pytest.mark.parametrize('variant', sorted(rc.table_cases()))
def test_committed_distances_match_recomputation(variant):
    found = rc.recompute_dist(variants=(variant,))[variant]
    assert sorted(found) == sorted(rc.DIST_REF[variant]), (sorted(found), sorted(rc.DIST_REF[variant]))
    for P, row in found.items():
        for k in rc.COMP:
            for q, got, committed in zip(rc.QC, row[k], rc.DIST_REF[variant][P][k]):
                print(variant, P, k, q, f'{got:.3e}', f'{committed:.3e}')
                assert got <= committed <= 2.0 * got, (variant, P, k, q, got, committed)


def test_table_covers_every_case_of_the_checks():
    for v in ('d1', 'd1e-3'):
        assert sorted(rc.DIST_REF[v]) == list(range(1, 17))
    for v in oc.SCHEDULES:
        assert sorted(rc.DIST_REF[v]) == sorted(oc.SCHEDULE_SIZES)
    assert sorted(rc.DIST_REF) == sorted(rc.table_cases())
    for rows in rc.DIST_REF.values():
        for row in rows.values():
            assert sorted(row) == ['n', 's'] and all(len(row[k]) == 2 and min(row[k]) > 0 for k in row)


def test_scene_parts_add_up():
    """S, N complex64, X = complex64(S + N) with the z rows included; masks and activity are online_checks.scene's own draws."""
    d = rc.scene_parts(11, 2, 4, 2, 6, True)
    X0, Z0, mask0 = oc.scene(11, 2, 4, 2, 6, True)
    assert np.array_equal(d['mask'], mask0)
    for a, b, c in ((d['X'], d['S'], d['N']), (d['Z'], d['Zs'], d['Zn'])):
        assert a.dtype == b.dtype == c.dtype == np.complex64 and np.array_equal(a, (b + c).astype(np.complex64))
    assert np.abs(d['X'] - X0).max() < 1e-6 * np.abs(X0).max() and np.abs(d['Z'] - Z0).max() < 1e-6 * np.abs(Z0).max()
    assert len({d['Zs'][1, j, 0, 5] for j in range(4)}) == 4 and len({d['Zn'][1, j, 0, 5] for j in range(4)}) == 4
    assert not np.array_equal(d['Zs'], d['Z']) and not np.array_equal(d['Zn'], d['Zs'])
    one = rc.scene_parts(11, 2, 1, 3, 6, False)
    assert one['Z'] is None and one['Zs'] is None and one['Zn'] is None
    assert np.all(np.abs(d['S'][:, :, 0]).max(axis=(1, 2, 3)) > 0)               # act[:, 0] = 1: the first solve sees the source
    full, cut = rc.RefCase('d1', 2, 3), rc.RefCase('d1', 2, 3, cut=(1, 5))
    for key, a in full.inputs().items():
        assert np.array_equal(a[:1, :, :5], cut.inputs()[key]), key


@pytest.mark.parametrize('M,K', [(4, 1), (4, 4), (8, 9)])
def test_every_reference_series_is_nonzero(M, K):
    """No problem needs to be skipped: y, s and n of every (room, node, bin) are non-zero (asserted inside reference())."""
    ref = rc.RefCase('d1', M, K).reference()
    assert ref['s'].shape == ref['n'].shape == ref['out'].shape


def test_restatement_with_companions_is_the_restatement():
    """out and w_last are online_checks.online_mwf_f32state's, bit for bit; a companion equal to the input gives `out`; the reference
    applied to S and N adds up to the reference's out, to the complex64 rounding of X = S + N."""
    c = rc.RefCase('u2', 3, 1, cut=(1, 8))
    V, m, VS, VN = c.problem_rows()
    p = c.oracle_params()
    out, w, (oy, os_, on_) = rc.online_mwf_f32state_comp(V, m, [V, VS, VN], **p)
    out0, w0 = oc.online_mwf_f32state(V, m, **p)
    assert rc.same(out, out0) and rc.same(w, w0) and rc.same(oy, out)
    assert os_.dtype == np.complex64 and not rc.same(os_, on_)
    ref = c.reference()
    o64, w_all = oo.online_mwf(V, m, **p)
    assert np.array_equal(o64, ref['out'])
    assert np.abs(ref['s'] + ref['n'] - ref['out']).max() < 1e-5 * np.abs(ref['out']).max()       # X is complex64(S + N): one rounding per entry
    # the filter in force: with update_every = 2 frame 1 is filtered with frame 0's filter, not its own
    assert np.array_equal(w_all[:, 1], w_all[:, 0]) and not np.array_equal(w_all[:, 2], w_all[:, 1])
    d = rc.comp_distances(os_, ref['s'])
    assert set(d) == set(rc.QC) and 0 < d['frame'].max() < 1e-4
