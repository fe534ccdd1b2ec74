"""The reference side of the covariance-route checks (tests/cov_checks.py), no GPU and no kernel: the route table is the dispatch of
api_cov.hip / api_step2_cov.hip (the shape tables are read out of the headers), the case list launches every instantiation a staged
call can reach and names the ones it cannot, the committed kernel trace of tests/test_gpu_cov_routes.py holds every reachable name, the
scenes are exact (float32 accumulation in NumPy equals the float64 sums bit for bit), and the helpers that lay z rows out say what
include/disco_hip.h says."""
import os
import re

import numpy as np

import cov_checks as cc
import room_checks as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'disco_amd', 'csrc')


def _read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _table(text, macro):
    body = re.search(r'#define\s+' + macro + r'\(X_\)((?:[^\n]*\\\n)*[^\n]*)', text).group(1)
    return tuple((int(a), int(b)) for a, b in re.findall(r'X_\((\d+),\s*(\d+)\)', body))


def test_shape_tables_are_the_headers():
    tables = _read(CSRC, 'dispatch.h')
    assert _table(tables, 'DISCO_FOR_MKR') == cc.MKR and len(cc.MKR) == 36
    got = _table(tables, 'DISCO_FOR_SPLIT_M8') + _table(tables, 'DISCO_FOR_SPLIT_M4') + _table(tables, 'DISCO_FOR_SPLIT_M2')
    assert sorted(got) == sorted(cc.SPLIT) and len([s for s in got if s[1] > 0]) == 24
    assert int(re.search(r'constexpr int CB_PMAX = (\d+);', _read(CSRC, 'k_cov.h')).group(1)) == cc.CB_PMAX
    assert int(re.search(r'CW_PMAX = (\d+);', _read(CSRC, 'k_cov_wide.h')).group(1)) == cc.CW_PMAX


def test_route_restates_the_dispatch_order():
    """The statements of api_cov.hip `route` leans on, in the order it assumes: refusals, the wide route, the split test, the (M, KR)
    table (taken only when the split test fails), the split kernels, k_cov_big.  The source lines are pinned verbatim ON PURPOSE: this is a
    drift alarm.  Whoever reorders or rewrites the dispatcher is sent here to restate the change in cov_checks.route, on which the coverage
    claim of the whole tier rests."""
    api = _read(CSRC, 'api_cov.hip')
    marks = ['if (M > 8) return fail', 'if (P > CW_PMAX) return fail', 'if (P > CB_PMAX) return cov_partials_wide',
             'const bool split = (KR == 0 || (P > 8 && same && mask_remote && (ctx->F - 1) % 64 == 0)) && cov_split_shape(M, KR);',
             'const bool mkr = !split && for_mkr(M, KR, [&](auto m, auto kr) {', 'if (!mkr) {', 'if (split)',
             'launch_cov_split_shape(M, KR, skiploc, (unsigned)nblk, st, a);', 'k_cov_big<SAMEZ>']
    at = [api.index(m) for m in marks]
    assert at == sorted(at)
    assert api.count('with_bool(KR == 0 || same, [&](auto samez) {') == 2 and 'with_bool(Zs == Zn, [&](auto samez) {' in api
    assert 'k_cov<M_, KR_, SAMEZ, NT>' in api and 'k_cov_wide<SAMEZ>' in api and api.count('constexpr bool SAMEZ = decltype(samez)::value;') == 3 and 'NT = decltype(n512)::value ? 320 : 576;' in api
    launch = _read(CSRC, 'cov_split_launch.h')
    assert 'k_cov_loc_f64<M>' in launch and 'k_cov_split_lds<M, KR, SKIP>' in launch and 'constexpr bool SKIP = KR > 0 && decltype(skip)::value;' in launch
    step2 = _read(CSRC, 'api_step2_cov.hip')
    assert 'if (P > 8) return fail' in step2 and 'k_step2_cov_fused<M_, K_, SKIPLOC, PACK>' in step2 \
        and 'for_mkr(M, K - 1, [&](auto m, auto kr) {' in step2 and 'K_ = decltype(kr)::value + 1;' in step2
    stft = _read(CSRC, 'api_stft_cov.hip')
    assert 'if (c.n_fft == 1024 && M > 6)' in stft
    # spot values
    assert cc.route(7, 1, 512, False) == ('k_cov_loc_f64<7>',) and cc.route(8, 1, 1024, False) == ('k_cov_loc_f64<8>',)
    assert cc.route(6, 1, 1024, False) == ('k_cov<6,0,true,576>',)
    assert cc.route(2, 3, 512, True, same_z=False) == ('k_cov<2,2,false,320>',)
    assert cc.route(8, 2, 512, True) == ('k_cov_split_lds<8,1,false>',)
    assert cc.route(8, 2, 512, True, same_z=False) == ('k_cov_big<false>',) and cc.route(8, 2, 512, True, mask_remote=False) == ('k_cov_big<true>',)
    assert cc.route(7, 3, 512, True) == ('k_cov_big<true>',) and cc.route(1, 16, 512, True) == ('k_cov_big<true>',)
    assert cc.route(1, 17, 512, True, same_z=False) == ('k_cov_wide<false>',) and cc.route(8, 25, 512, True) == ('k_cov_wide<true>',)
    assert cc.route(8, 26, 512, True)[0].startswith('refused') and cc.route(9, 1, 512, False)[0].startswith('refused')
    assert cc.route(7, 1, 1024, False, call='stft_cov') == ('k_stft', 'k_cov_loc_f64<7>') and cc.route(7, 1, 512, False, call='stft_cov') == ('k_stft_cov<512,7,true>',)
    assert cc.route(4, 5, 512, True, call='step2_fused') == ('k_step2_cov_fused<4,5,false>',) and cc.route(4, 6, 512, True, call='step2_fused')[0].startswith('refused')


def test_case_list_launches_every_reachable_instantiation():
    reach = cc.reachable()
    launched = cc.launched_by(cc.exact_cases()) | {f'k_step2_cov_fused<{M},{K},true>' for M, K in cc.reuse_shapes()} \
        | rc.launched_by(rc.staged_cases())
    assert launched == reach, (sorted(reach - launched), sorted(launched - reach))
    # 2 FFT sizes x (6 step-1 + 28 step-2 x 2) k_cov, 2 k_cov_loc_f64, 24 k_cov_split_lds, 2 + 2, 36 + 28 fused; through the test-only entry
    # the 24 k_cov_split_lds<.., true> and the 6 shapes of the room pass
    assert len(reach) == 2 * (6 + 56) + 2 + 24 + 4 + 36 + 28 + 24 + 6
    assert cc.reachable(selftest=False) | cc.selftest_reachable() == reach and not cc.reachable(selftest=False) & cc.selftest_reachable()
    # the staged calls alone launch what they launched before, and the new cases launch every name the test-only entry adds -- by themselves
    assert cc.launched_by(cc.exact_cases()) | {f'k_step2_cov_fused<{M},{K},true>' for M, K in cc.reuse_shapes()} == cc.reachable(selftest=False)
    assert cc.selftest_reachable() <= rc.launched_by(rc.staged_cases())
    assert {(M, K) for M, K, _t in rc.reuse_cases()} == set(cc.reuse_shapes())
    # what the (M, KR) table instantiates and no staged call reaches is listed as such: k_cov<7, 0>, k_cov<8, 0> sit behind
    # k_cov_loc_f64 ((7, 0) and (8, 0) are split shapes and the split test comes first), and a step-1 call never has distinct Zn
    inst = {f'k_cov<{M},{KR},{s},{nt}>' for M, KR in cc.MKR for s in ('true', 'false') for nt in (320, 576)}
    assert inst - reach == set(cc.UNREACHABLE)
    assert all(cc.route(M, 1, n, False) == (f'k_cov_loc_f64<{M}>',) for M in (7, 8) for n in (512, 1024))
    # every P of 9 .. 16 through both k_cov_big forms, every P of 17 .. 32 through k_cov_wide<true>
    big = {(cc.route(c['M'], c['K'], c['n_fft'], True, c['same_z'], c['mask_remote'])[0], c['M'] + c['K'] - 1)
           for c in cc.exact_cases() if c['call'] == 'cov_masked' and c['step2']}
    for P in range(9, 17):
        assert ('k_cov_big<true>', P) in big and ('k_cov_big<false>', P) in big, P
    for P in range(17, 33):
        assert ('k_cov_wide<true>', P) in big, P
    assert sum(1 for n, P in big if n == 'k_cov_wide<false>') >= 3
    assert set(cc.CASE_FAMILIES) == {cc.family_of(c) for c in cc.exact_cases()}


def test_geometry_holds_the_chunk_lengths_the_issue_names():
    lens = {n for T, c in cc.GEOMETRY for n in cc.chunk_lengths(T, c if c else 8)}
    assert {64, 65, 129, 626} <= lens
    assert {T for T, _ in cc.GEOMETRY} >= {1, 2, 3, 63, 64, 65, 129, 626}
    assert {c for _, c in cc.GEOMETRY} >= {1, 2, 3, 7, 8} and any(c > T for T, c in cc.GEOMETRY)
    assert any(c and T % c for T, c in cc.GEOMETRY) and (626, 1) in cc.GEOMETRY
    assert any(max(cc.chunk_lengths(T, c)) > 64 for T, c in cc.GEOMETRY_CUT)


def test_committed_kernel_trace_holds_every_reachable_name():
    lines = [l for l in _read(REPO, 'profiles', 'cov_routes_kernels.txt').splitlines() if l.strip() and not l.startswith('#')]
    traced = {cc.kernel_key(l) for l in lines}
    stft = {n for M in range(1, 9) for n_fft in (512, 1024) for n in cc.route(M, 1, n_fft, False, call='stft_cov') if n != 'k_stft'}
    assert len(stft) == 14 + 2                   # k_stft_cov<512, 1 .. 8>, <1024, 1 .. 6>; the staged pair ends in k_cov_loc_f64<7>, <8>
    missing = sorted((cc.reachable(selftest=False) | stft) - traced)     # (the trace is of tests/test_gpu_cov_routes.py: the staged calls)
    assert not missing, missing
    assert not traced & set(cc.UNREACHABLE), sorted(traced & set(cc.UNREACHABLE))


def test_scenes_are_exact():
    """The representability bound holds for the longest and the widest scenes (ref_sums asserts it for every case it builds), and a
    frame-by-frame float32 accumulation in NumPy equals the float64 sums bit for bit."""
    for (M, K, step2), T in [((2, 3, True), 626), ((7, 1, False), 626), ((3, 8, True), 626), ((2, 17, True), 626), ((8, 25, True), 64)]:
        X, Zs, Zn, mask = cc.scene(3, 1, K, M, T, 33, step2)
        assert X.dtype == np.complex64 and mask.dtype == np.float32 and set(np.unique(mask)) <= set(cc.MASK_VALUES)
        assert np.array_equal(X.real, np.round(X.real)) and np.abs(X.real).max() <= 3 and np.abs(X.imag).max() <= 3
        for mr, zn in ((True, Zs), (False, Zn)):
            Sss, Snn = cc.ref_sums(X, mask, Zs, zn, mr)
            P = M + (K - 1 if step2 else 0)
            assert Sss.shape == Snn.shape == (1, K, 33, P, P)
    X, _zs, _zn, mask = cc.scene(4, 2, 2, 4, 626, 33, False)
    assert (mask == 0).all(axis=2).any() and (mask == 1).all(axis=2).any()       # whole bins of exact 0 and of exact 1
    Sss, Snn = cc.ref_sums(X, mask)
    for r, k, f in ((0, 0, 0), (1, 1, 32), (0, 1, 17), (1, 0, 5)):
        ss, nn = cc.f32_sequential_sums(X, mask, r, k, f)
        assert ss.dtype == np.complex64 and np.array_equal(ss.astype(np.complex128), Sss[r, k, f])
        assert np.array_equal(nn.astype(np.complex128), Snn[r, k, f])
    # the bound is a real assertion: a scene 400 times as strong breaks it
    try:
        cc.ref_sums(X * 400, mask)
    except AssertionError as e:
        assert 'representability' in str(e)
    else:
        raise AssertionError('the bound did not fire')


def test_mean_tolerance_is_the_two_roundings():
    """float32(S * float64(float32(1) / float32(T))) against S / T: inside 1.01 x 2^-23 for every T of the geometry, exact for powers of two."""
    rng = np.random.default_rng(0)
    S = rng.integers(-2 ** 20, 2 ** 20, 20000).astype(np.float64) / 16
    for T in sorted({T for T, _ in cc.GEOMETRY} | {37, 16, 61}):
        got = (S * np.float64(np.float32(1) / np.float32(T))).astype(np.float32).astype(np.float64)
        err = np.abs(got - S / T)
        assert (err <= cc.MEAN_TOL * np.abs(S / T)).all(), T
        if T & (T - 1) == 0:
            assert (err == 0).all(), T
    assert (np.float64(0.0) * np.float64(np.float32(1) / np.float32(3))) == 0


def test_compare_exact_sees_one_wrong_entry():
    X, Zs, _zn, mask = cc.scene(1, 2, 3, 2, 64, 9, True)
    Sss, _ = cc.ref_sums(X, mask, Zs, Zs)
    good = (Sss / 64).astype(np.complex64)
    cc.compare_exact(good, Sss, [64, 64], 'good')
    for what, edit in (('one entry one ulp', lambda a: a.__setitem__((1, 2, 4, 0, 3), np.nextafter(a[1, 2, 4, 0, 3].real, np.float32(9)) + 1j * a[1, 2, 4, 0, 3].imag)),
                       ('mirror not conjugated', lambda a: a.__setitem__((0, 1, 8, 2, 1), a[0, 1, 8, 1, 2])),
                       ('imaginary diagonal', lambda a: a.__setitem__((0, 0, 0, 1, 1), a[0, 0, 0, 1, 1] + np.complex64(1e-30j)))):
        bad = good.copy()
        edit(bad)
        try:
            cc.compare_exact(bad, Sss, [64, 64], what)
        except AssertionError:
            continue
        raise AssertionError(f'compare_exact did not see: {what}')


def test_layout_helpers_follow_the_header():
    hdr = _read(REPO, 'include', 'disco_hip.h')
    assert '[W][R][nodes_per_block][T][F]' in hdr and 'v_s(t,f) = [ m*X_k ; g_s*Zs_j (j<k) ; g_s*Zs_j (j>k) ]' in hdr
    assert 'return ((long long)(j / zblk) * R + r) * zblk + (j % zblk);' in _read(CSRC, 'common.h')
    R, K, T, F = 3, 6, 2, 5
    Z = (np.arange(R * K * T * F).reshape(R, K, T, F) + 0j).astype(np.complex64)
    for zblk in (1, 2, 3, 6):
        B = cc.z_to_blocks(Z, zblk)
        assert B.shape == (K // zblk, R, zblk, T, F)
        planes = B.reshape(R * K, T, F)
        for r in range(R):
            for j in range(K):
                assert np.array_equal(planes[cc.z_plane(r, j, R, zblk)], Z[r, j])
    assert np.array_equal(cc.z_to_blocks(Z, K)[0], Z)
    # rows of node k: its own channels, then z_j for j < k, then j > k; a node subset keeps global z indices
    X = (np.arange(R * 2 * T * F * 2).reshape(R, 2, T, F, 2) * 1j).astype(np.complex64)
    v = cc.rows_of(X, Z, 1, 4, 1)
    assert v.shape == (T, F, 2 + K - 1) and np.array_equal(v[..., :2], X[1, 1])
    assert [int(v[0, 0, 2 + i].real) for i in range(K - 1)] == [int(Z[1, j, 0, 0].real) for j in (0, 1, 2, 3, 5)]


def test_committed_float_distances_match_recomputation():
    found = cc.recompute_float_dist()
    assert sorted(found) == sorted(cc.FLOAT_DIST) == sorted(cc.FLOAT_SHAPES)
    for fam, row in found.items():
        for q, got, committed in zip(('fro', 'coh'), row, cc.FLOAT_DIST[fam]):
            print(fam, q, f'{got:.3e}', f'{committed:.3e}')
            assert got <= committed <= 2.0 * got, (fam, q, got, committed)
    # the families of the float tier are the families of the exact tier, on their own routes
    for fam, (M, K, step2) in cc.FLOAT_SHAPES.items():
        assert cc.route(M, K, 512, step2)[0].startswith(fam + '<'), fam


def test_restatement_rounds_and_the_reference_does_not():
    X, Z, mask = cc.float_scene('k_cov', T=40, F=9)
    rs, rn = cc.float_ref(X, Z, mask)
    a, b = cc.cov_f32_restatement(X, Z, mask)
    a3, b3 = cc.cov_f32_restatement(X, Z, mask, chunks=3)
    assert a.dtype == np.complex64 and a.shape == rs.shape
    for got, ref in ((a, rs), (b, rn), (a3, rs), (b3, rn)):
        fro, coh = cc.pencil_quantities(got, ref)
        assert 1e-9 < fro.max() < 2e-6 and fro.max() <= coh.max() * ref.shape[-1] and coh.max() < 5e-6
    assert not np.array_equal(a, a3)
    # one wrong small entry: coh sees what fro averages away
    bad = rs.copy()
    small = np.unravel_index(np.argmin(np.abs(rs[0, 0, 4]) + 10 * np.eye(rs.shape[-1])), rs.shape[-2:])
    bad[0, 0, 4][small] *= 1.5
    fro, coh = cc.pencil_quantities(bad, rs)
    assert coh[0, 0, 4] > 2 * fro[0, 0, 4] / rs.shape[-1] and coh[0, 0, 4] > 0 and fro[0, 0, 3] == 0


def test_committed_stft_distances_match_recomputation():
    found = cc.recompute_stft_dist()
    assert sorted(found) == sorted(cc.STFT_DIST) == sorted(cc.stft_cases())
    for cid, row in found.items():
        for q, got, committed in zip(('fro', 'coh'), row, cc.STFT_DIST[cid]):
            assert got <= committed <= 2.0 * got, (cid, q, got, committed)
    cases = cc.stft_cases().values()
    # the cases the transform's tier has to hold: every instantiation, both pad modes, the named runs, short clips, lengths
    names = {cc.route(c['M'], 1, c['n_fft'], False, call='stft_cov') for c in cases}
    assert names == {(f'k_stft_cov<512,{M},true>',) for M in range(1, 9)} | {(f'k_stft_cov<1024,{M},true>',) for M in range(1, 7)} \
        | {('k_stft', 'k_cov_loc_f64<7>'), ('k_stft', 'k_cov_loc_f64<8>')}
    assert {c['pad'] for c in cases} == {'reflect', 'constant'} and {c['runw'] for c in cases} >= {8, 40, 79, 80, 400}
    assert {c['T'] for c in cases} >= {2, 3} and any(c['runw'] > c['T'] for c in cases) and sum(c['frames'] is not None for c in cases) >= 3
    assert any(c['runw'] and c['T'] % (4 * c['runw']) and c['T'] % (4 * c['runw']) <= c['runw'] for c in cases)      # empty waves at the end


def test_room_tables_and_staged_step2_restate_the_host_code():
    """The tables and the route rule of tests/room_checks.py against dispatch.h / api_room.hip / api_path.hip / api_cov.hip; the source
    lines are pinned verbatim on purpose (a drift alarm, as in test_route_restates_the_dispatch_order)."""
    tables = _read(CSRC, 'dispatch.h')
    assert _table(tables, 'DISCO_FOR_ROOM') == cc.ROOM == rc.ROOM
    assert 'k_room_cov_dma<M_, K_, 8>' in _read(CSRC, 'api_room_s8.hip') and rc.ROOM_SUB == 8
    assert int(re.search(r'constexpr int ROOM_DEPTH = (\d+);', _read(CSRC, 'k_room.h')).group(1)) == rc.ROOM_DEPTH
    assert len(rc.SPLIT_SHAPES) == 24 and all(8 < M + K - 1 <= cc.CB_PMAX for M, K in rc.SPLIT_SHAPES)
    path = _read(CSRC, 'api_path.hip')
    marks = ['int staged_step2(disco_ctx* ctx,', 'if (same_mask && room_cov_ok(ctx, X, mask_w)) {', 'room_cov_partials(ctx, X, mask_w, w_loc, z, s, store_z)',
             'disco_apply(ctx, X, nullptr, w_loc, c.mics, 1, z, s)', 'cov_partials(ctx, X, mask_w, zr, zr, 1, c.mics + c.nodes - 1, s, same_mask && c.nodes > 1)',
             'static void push_staged_step2(', 'return staged_step2(ctx, X, mask_w, same_mask, w_loc, z, store_z, s);',
             'extern "C" int disco_selftest_staged_step2(', 'cov_partials(ctx, X, mask, nullptr, nullptr, 1, ctx->cfg.mics, s);',
             'return staged_step2(ctx, X, mask, true, w_loc, z, store_z != 0, s, route_out);']
    at = [path.index(m) for m in marks]
    assert at == sorted(at)
    assert path.count('room_cov_partials(') == 1 and path.count('staged_step2(ctx, X, mask') == 2      # ONE body behind the whole path and the entry
    room = _read(CSRC, 'api_room.hip')
    assert 'if (!want || !shape || M + K - 1 <= 8 || sharded(ctx) || !X || !mask) return false;' in room
    assert 'skiploc = skiploc && split && KR > 0 && step1_held(ctx, X, mask);' in _read(CSRC, 'api_cov.hip')
    hdr = _read(REPO, 'include', 'disco_hip.h')
    from disco_amd.engine import Engine
    for name, code in (('ROOM', 'room'), ('SPLIT_SKIPLOC', 'split_skiploc'), ('WHOLE', 'whole')):
        n = int(re.search(r'#define DISCO_STAGED_ROUTE_' + name + r' (\d+)', hdr).group(1))
        assert Engine.STAGED_ROUTES[n] == code
    # spot values
    assert rc.expected_route(8, 8, 1) == 'room' and rc.expected_route(8, 8, 0) == 'split_skiploc' and rc.expected_route(4, 4, 1) == 'whole'
    assert rc.expected_route(2, 8, 1) == 'split_skiploc' and rc.expected_route(3, 8, 0) == 'whole' and rc.expected_route(2, 16, 0) == 'whole'
    assert rc.kernel_of(4, 6, 512, 1) == 'k_room_cov_dma<4,6,8>' and rc.kernel_of(4, 6, 512, 0) == 'k_cov_split_lds<4,5,true>'


def test_room_cases_hold_what_the_checks_claim():
    """The shapes and edges of the staged-step-2 tier, counted on the case list itself."""
    cases = rc.staged_cases()
    room = [c for c in cases if rc.expected_route(c['M'], c['K'], c['room_cov']) == 'room']
    split = [c for c in cases if rc.expected_route(c['M'], c['K'], c['room_cov']) == 'split_skiploc']
    assert len(room) + len(split) == len(cases)
    assert {(c['M'], c['K'], c['n_fft']) for c in room} == {(M, K, n) for M, K in rc.ROOM for n in (512, 1024)}
    assert {(c['M'], c['K']) for c in split} >= set(rc.SPLIT_SHAPES) and any(c['n_fft'] == 1024 for c in split)
    for M, K in ((8, 2), (4, 6)):                                          # every frame count around the ring on these two
        assert {c['T'] for c in room if (c['M'], c['K'], c['n_fft'], c['R']) == (M, K, 512, 1)} >= set(rc.RING_T)
    assert set(rc.RING_T) == {1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49}
    for M, K in rc.ROOM:
        assert {c['T'] for c in room if (c['M'], c['K']) == (M, K)} >= set(rc.RING_T_SUBSET)
    # item walking: 65 tiles per room at 512 points over min(items, CUs) workgroups rounded down to a multiple of 64
    def walks(R, tiles=65, cus=256):
        items = R * tiles
        nwg = min(items, cus)
        nwg = max(64, nwg // 64 * 64) if items >= 64 else nwg
        return -(-items // nwg)
    assert [walks(R) for R in (1, 2, 8)] == [2, 2, 3]
    assert {c['R'] for c in room if c['n_fft'] == 512 and not c.get('frames')} >= {1, 2, 8}
    lens = [c for c in room if c.get('frames')]
    assert any(c['R'] == 8 for c in lens) and all(max(c['frames']) == c['T'] for c in lens)
    assert any(a == 1 and b == c['T'] or a == c['T'] and b == 1 for c in lens for a, b in zip(c['frames'], c['frames'][1:]))   # one frame next to a full room
    assert sum(c.get('store_z') is False for c in room) >= 3
    # the split route: frame counts either side of its chunk boundaries, fewer frames than chunks, lengths
    geo = {(c['T'], c.get('chunks', 0)) for c in split}
    assert geo >= set(rc.SPLIT_GEOMETRY) and {(15, 2), (16, 2), (17, 2), (31, 4), (32, 4), (33, 4)} <= geo and any(ch > T for T, ch in geo)
    assert any(c.get('frames') for c in split)
    # pending solves (every room >= 4 P frames) on both routes, P = 9 and beyond
    solved = [c for c in cases if min(c.get('frames') or (c['T'],)) >= 4 * (c['M'] + c['K'] - 1)]
    assert {c['room_cov'] for c in solved} == {0, 1} and len({c['M'] + c['K'] - 1 for c in solved}) >= 3
    assert max(c['T'] for c in cases) <= 49
    assert len({rc.case_id(c) for c in cases}) == len(cases)


def test_room_filters_and_scenes_are_exact():
    """Two or three taps from {+-1, +-i, +-1 +- i}; z = w^H x is an integer and the representability bound holds at the longest and the widest
    cases (ref_sums asserts it on every case the checks build)."""
    w = rc.room_filters(3, 2, 8, 33, 8)
    nz = (w != 0).sum(axis=-1)
    assert nz.min() >= 1 and nz.max() == 3 and (nz >= 2).mean() > 0.8
    assert set(np.unique(w[w != 0])) <= set(rc.TAPS) and len(set(np.unique(w[w != 0]))) == 8
    for M, K, T in ((8, 8, 49), (4, 8, 49), (2, 15, 49), (8, 9, 49)):
        X, _zs, _zn, mask = cc.scene(5, 1, K, M, T, 17, False)
        z = rc.exact_z(X, rc.room_filters(7, 1, K, 17, M))
        assert np.array_equal(z, np.round(z.real) + 1j * np.round(z.imag)) and np.abs(z.real).max() <= 18
        zc = z.astype(np.complex64)
        assert np.array_equal(zc.astype(np.complex128), z)
        Sss, Snn = cc.ref_sums(X, mask, zc, zc, True)
        assert Sss.shape == (1, K, 17, M + K - 1, M + K - 1)
