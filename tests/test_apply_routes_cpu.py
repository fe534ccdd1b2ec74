"""The reference side of the filter-and-sum / inverse-transform checks (tests/apply_checks.py), no GPU and no kernel: the route table is
the dispatch of api_apply.hip, api_step2_apply.hip, api_step2_istft.hip, api_apply_istft_wide.hip and istft_any (the shape tables and
the LDS budget are read out of the sources), the case lists launch every instantiation an ABI call can reach and name the ones it
cannot, the committed kernel trace of tests/test_gpu_apply_routes.py holds every reachable name, the scenes are exact, the comparisons
see one wrong output, and the float32 restatement behind the inverse-transform bar rounds where the float64 oracle does not."""
import os
import re

import numpy as np

import apply_checks as ac
import cov_checks as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'disco_amd', 'csrc')


def _read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _table(text, macro):
    body = re.search(r'#define\s+' + macro + r'\(X_\)((?:[^\n]*\\\n)*[^\n]*)', text).group(1)
    return tuple((int(a), int(b)) for a, b in re.findall(r'X_\((\d+),\s*(\d+)\)', body))


def test_shape_tables_are_the_sources():
    tables = _read(CSRC, 'dispatch.h')
    assert _table(tables, 'DISCO_FOR_MKR') == ac.MKR and len(ac.MKR) == 36
    assert _table(tables, 'DISCO_FOR_ROOM') == ac.ROOM
    body = re.search(r'#define DISCO_FOR_WIDE_ISTFT\(X_\) DISCO_FOR_ROOM\(X_\)([^\n]*)', tables).group(1)
    assert ac.ROOM + tuple((int(a), int(b)) for a, b in re.findall(r'X_\((\d+),\s*(\d+)\)', body)) == ac.WIDE_ISTFT and len(ac.WIDE_ISTFT) == 9
    api = _read(CSRC, 'api_apply.hip')
    assert _table(tables, 'DISCO_FOR_APPLY_MQ') == ac.MQ and 'for_apply_mq(M, krt, [&](auto m, auto k) {' in api
    assert 'const int krt = KR <= 1 ? 1 : (KR <= 3 ? 3 : (KR <= 7 ? 7 : 15));' in api
    assert [ac.krt_of(kr) for kr in range(1, 16)] == [1, 3, 3] + [7] * 4 + [15] * 8
    # the LDS budget and the struct it is held against, member by member
    istft = _read(CSRC, 'api_step2_istft.hip')
    assert 'constexpr bool apply_istft_fits = sizeof(ApplyIstftShared<512, M, K>) <= 160 * 1024;' in istft and ac.LDS_BUDGET == 160 * 1024
    assert istft.count('apply_istft_fits<') == 2              # the predicate and the launch
    fused = _read(CSRC, 'k_fused.h')
    struct = re.search(r'struct alignas\(16\) ApplyIstftShared \{(.*?)\};', fused, re.S).group(1)
    assert [l.split(';')[0].strip() for l in struct.strip().splitlines()] == [
        'c32 buf[K][fft_buf_len<N>()]', 'c32 zbuf[2][K][K > 1 ? N / 2 + 1 : 1]', 'c32 wl[K][K > 1 ? N / 2 + 1 : 1][M]']
    fft = _read(CSRC, 'fft.h')
    assert 'constexpr int fft_buf_len() { return N + (N >> FftPlan<N>::PADSH); }' in fft and 'static constexpr int E = 8, PADSH = 3' in fft
    assert ac.apply_istft_shared_bytes(4, 4) == 8 * (4 * 576 + 2 * 4 * 257 + 4 * 257 * 4) and ac.apply_istft_shared_bytes(3, 1) == 8 * (576 + 2 + 3) + 8
    sizes = {s: ac.apply_istft_shared_bytes(*s) for s in ac.fused_shapes()}
    assert max(sizes.values()) == sizes[(2, 7)] == 89824 < ac.LDS_BUDGET        # all 36 fit: the refusal branch of the budget is dead today


def test_route_restates_the_dispatch_order():
    """The statements of the dispatchers `route` leans on, in the order it assumes.  Pinned verbatim ON PURPOSE: a drift alarm.  Whoever
    reorders a dispatcher is sent here to restate the change in apply_checks.route, on which the coverage claim of the tier rests."""
    api = _read(CSRC, 'api_apply.hip')
    marks = ['if (KR != 0 && KR != c.nodes - 1) return fail', 'if (M > 8) return fail', 'if (P > 32) return fail',
             'const bool flat = for_mkr(M, KR, [&](auto m, auto kr) {', 'if (flat) return check_launch',
             'if ((M == 4 || M == 8) && KR >= 1 && KR <= 15) {', 'if (KR > 15) {', 'k_apply_m<decltype(m)::value, 31>', 'k_apply_m<decltype(m)::value>)']
    at = [api.index(m) for m in marks]
    assert at == sorted(at)
    assert api.count('for_int<1, 8>(M, [&](auto m) {') == 2 and 'template <int M, int KRMAX = 15>' in _read(CSRC, 'k_apply.h')
    s2 = _read(CSRC, 'api_step2_apply.hip')
    marks = ['if (sharded(ctx)) return fail', 'if (P > 8) return fail', 'for_mkr(M, K - 1, [&](auto m, auto kr) {', 'K_ = decltype(kr)::value + 1;',
             'k_step2_apply_fused<M_, K_>']
    assert [s2.index(m) for m in marks] == sorted(s2.index(m) for m in marks)
    si = _read(CSRC, 'api_step2_istft.hip')
    marks = ['if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED', 'if (c.n_fft != 512 || P > 8) return fail',
             'for_mkr(M, K - 1, [&](auto m, auto kr) { with_bool(layout == XLayout::Packed', 'K_ = decltype(kr)::value + 1;',
             'if constexpr (apply_istft_fits<M_, K_> && (!PACK || K_ >= 2)) {', 'k_step2_apply_istft<512, M_, K_, PACK>']
    assert [si.index(m) for m in marks] == sorted(si.index(m) for m in marks)
    wide = _read(CSRC, 'api_apply_istft_wide.hip')
    assert 'if (!wide_istft_shape(ctx->cfg)) return fail(ctx, DISCO_E_UNSUPPORTED' in wide and 'constexpr int N = decltype(n1024)::value ? 1024 : 512, M_ = decltype(m)::value, KR_ = decltype(k)::value - 1;' in wide \
        and 'k_apply_istft_wide<N, M_, KR_>' in wide and 'for_wide_istft(c.mics, K, [&](auto m, auto k) {' in wide and 'const int K = c.nodes, WV = c.n_fft / 256;' in wide
    stft = _read(CSRC, 'api_stft.hip')
    assert 'return istft_any(ctx, Z, n_sig, out, ctx->cfg.length, ctx->T, s, false, ctx->d_lens, spr);' in stft and 'k_istft<N, SOLO>' in stft
    assert 'constexpr int ISTFT_SEGS = ISTFT_FRAMES - 1;' in _read(CSRC, 'k_stft.h')
    # spot values
    r = ac.route
    assert r(4, 5, 512, 'apply') == ('k_apply<4,4>',) and r(4, 6, 512, 'apply') == ('k_apply_mq<4,7>',) and r(4, 17, 512, 'apply') == ('k_apply_m<4,31>',)
    assert r(8, 2, 512, 'apply') == ('k_apply_mq<8,1>',) and r(8, 2, 512, 'apply', step2=False) == ('k_apply<8,0>',)
    assert r(7, 3, 512, 'apply') == ('k_apply_m<7,15>',) and r(1, 9, 1024, 'apply') == ('k_apply_m<1,15>',) and r(1, 17, 512, 'apply') == ('k_apply_m<1,31>',)
    assert r(8, 26, 512, 'apply')[0].startswith('refused') and r(9, 1, 512, 'apply')[0].startswith('refused')
    assert r(4, 5, 1024, 'step2_fused') == ('k_step2_apply_fused<4,5>',) and r(4, 6, 512, 'step2_fused')[0].startswith('refused')
    assert r(2, 2, 512, 'step2_fused', sharded=True)[0].startswith('refused') and r(2, 2, 1024, 'step2_istft')[0].startswith('refused')
    assert r(2, 2, 512, 'step2_istft') == ('k_step2_apply_istft<512,2,2>',) and r(4, 3, 1024, 'apply_istft') == ('k_apply_istft_wide<1024,4,2>',)
    assert r(4, 5, 512, 'apply_istft')[0].startswith('refused') and r(3, 3, 1024, 'istft') == ('k_istft<1024,false>',)


def test_case_lists_launch_every_reachable_instantiation():
    reach = ac.reachable()
    exact, transform = ac.launched_by_exact(), ac.launched_by_istft()
    assert exact | transform == reach, (sorted(reach - exact - transform), sorted((exact | transform) - reach))
    # 36 k_apply, 6 k_apply_m<M, 15>, 8 k_apply_m<M, 31>, 6 k_apply_mq, 36 + 36 on-chip-z kernels, 18 k_apply_istft_wide, 2 k_istft
    assert len(reach) == 36 + 6 + 8 + 6 + 36 + 36 + 18 + 2
    assert ac.instantiated() - reach == set(ac.UNREACHABLE) and not reach - ac.instantiated()
    assert all(ac.route(4, kr + 1, 512, 'apply') == (f'k_apply<4,{kr}>',) for kr in range(1, 5))       # why k_apply_mq<4, 1>, <4, 3> are dead
    assert {n for n in reach if n.startswith('k_apply_m<') and n.endswith(',15>')} == {f'k_apply_m<{M},15>' for M in (1, 2, 3, 5, 6, 7)}
    # the filter outputs are exact on every filter kernel; the transform tier runs every kernel that transforms
    assert {n for n in reach if 'istft' not in n} <= exact and {n for n in reach if 'k_apply_istft_wide' in n} <= exact & transform
    assert {n for n in reach if 'istft' in n} <= transform
    # k_apply_mq: every KRT bucket that can hold KR < KRT has such a case (the padding rows run) and one with KR = KRT
    mq = {}
    for c in ac.apply_cases():
        name = ac.route(c['M'], c['K'], c['n_fft'], 'apply', step2=c['step2'])[0]
        if name.startswith('k_apply_mq'):
            mq.setdefault(name, set()).add(c['K'] - 1)
    for name, krs in mq.items():
        krt = int(name.split(',')[1][:-1])
        assert krt in krs and (krt == 1 or min(krs) < krt), (name, krs)
    # P = 32 and KR = 16 through k_apply_m<M, 31> for every M; both conj_w forms are check_apply's default
    wide = {(c['M'], c['K'] - 1) for c in ac.apply_cases() if c['K'] > 16}
    assert {(M, 16) for M in range(1, 9)} | {(M, 32 - M) for M in range(1, 9)} <= wide
    assert {c['T'] for c in ac.apply_cases()} == set(ac.T_DEFAULT) and {c['n_fft'] for c in ac.apply_cases()} == {512, 1024}
    import inspect
    assert inspect.signature(ac.check_apply).parameters['conjs'].default == (True, False)


def test_geometry_and_transform_cases_hold_what_the_tier_names():
    (M, K), Ts = ac.GEOM_APPLY['k_apply']                                  # T F against the cap of 64 blocks of 256
    blocks = [(T * 257 + 255) // 256 for T in Ts]
    assert min(blocks) < 64 and 64 in blocks and max(blocks) > 64
    for fam in ('k_apply_m', 'k_apply_mq'):
        Ts = ac.GEOM_APPLY[fam][1]
        assert any(T < 16 for T in Ts) and 16 in Ts and any(T >= 16 and T % 8 for T in Ts)
        assert any((max(1, T // 8) - 1) * -(-T // max(1, T // 8)) >= T for T in Ts)                 # an empty last chunk
    assert {T for T, _ in ac.GEOM_FUSED} >= {1, 63, 64, 65, 129} and {c for _, c in ac.GEOM_FUSED} >= {1, 2, 3} and any(c > T for T, c in ac.GEOM_FUSED)
    cases = ac.istft_cases()
    for entry, runs_per_wg in (('step2_istft', {512: 1}), ('apply_istft', {512: 2, 1024: 4})):
        mine = [c for c in cases if c['entry'] == entry and c['lengths'] is None]
        assert {c['pairs'] for c in mine} == {0, 2, 3, 4, 64}
        for n_fft, wv in runs_per_wg.items():
            for pairs in (2, 3, 4):
                span = wv * (2 * pairs - 1)
                segs = {-(-c['L'] // (n_fft // 2)) for c in mine if c['pairs'] == pairs and c['n_fft'] == n_fft}
                assert {span, span + 1} <= segs and any(s > span + 1 and s % (2 * pairs - 1) == 0 for s in segs), (entry, n_fft, pairs, segs)
        frames = {1 + c['L'] // (c['n_fft'] // 2) for c in mine}
        assert {2, 3} <= frames and any(t % 2 for t in frames) and any(t % 2 == 0 for t in frames)
        assert any(c['L'] % (c['n_fft'] // 2) == 0 for c in mine) and any(c['L'] % (c['n_fft'] // 2) for c in mine)
        assert any(c['staged'] for c in mine) and any(c['lengths'] for c in cases if c['entry'] == entry)
    assert all(c['L'] % (c['n_fft'] // 2) <= c['n_fft'] // 4 for c in cases)
    assert {-(-c['L'] // 256) for c in cases if c['entry'] == 'istft' and c['n_fft'] == 512} >= {7, 8, 14, 1, 2, 3}
    for c in cases:
        for Lr in c['lengths'] or ():
            assert Lr <= c['L'] and Lr % (c['n_fft'] // 2) <= c['n_fft'] // 4
    assert any(min(c['lengths']) < c['n_fft'] // 2 for c in cases if c['lengths'])                    # a one-frame room


def test_committed_kernel_trace_holds_every_reachable_name():
    traced = ac.trace_names(_read(REPO, 'profiles', 'apply_routes_kernels.txt'))
    missing = sorted(ac.reachable() - traced)
    assert not missing, missing
    assert not traced & set(ac.UNREACHABLE), sorted(traced & set(ac.UNREACHABLE))


def test_scenes_are_exact_and_comparisons_see_one_wrong_output():
    X, Z, w = ac.apply_scene(3, 2, 6, 4, 3, 33)
    assert X.dtype == Z.dtype == w.dtype == np.complex64 and np.array_equal(X.real, np.round(X.real)) and np.abs(X.real).max() == 8
    assert np.array_equal(w * 4, np.round(w.real * 4) + 1j * np.round(w.imag * 4)) and np.abs(w.imag).max() == 2
    assert (w == 0).all(axis=-1).any() and ((w == 0).any(axis=-1) & ~(w == 0).all(axis=-1)).any()      # all-zero filters, single zero taps
    ref = ac.ref_apply(X, Z, w)
    # a float32 accumulation in NumPy, one product at a time, equals the float64 sums bit for bit
    V = ac.rows_all(X, Z, range(6)).astype(np.complex64)
    acc = np.zeros(ref.shape, np.complex64)
    for p in range(w.shape[-1]):
        acc = (acc + (w[:, :, None, :, p].conj() * V[..., p]).astype(np.complex64)).astype(np.complex64)
    ac.compare_bits(acc, ref, 'float32 accumulation')
    assert not np.array_equal(ac.ref_apply(X, Z, w, conj=False), ref)
    for what, edit in (('one output one ulp', lambda a: a.__setitem__((1, 5, 2, 32), np.nextafter(a[1, 5, 2, 32].real, np.float32(1e9)) + 1j * a[1, 5, 2, 32].imag)),
                       ('one imaginary sign', lambda a: a.__setitem__((0, 0, 0, 7), np.conj(a[0, 0, 0, 7]) if a[0, 0, 0, 7].imag else a[0, 0, 0, 7] + 1j)),
                       ('a NaN', lambda a: a.__setitem__((1, 0, 1, 0), np.nan))):
        bad = acc.copy()
        edit(bad)
        try:
            ac.compare_bits(bad, ref, what)
        except AssertionError:
            continue
        raise AssertionError(f'compare_bits did not see: {what}')
    # the faults the tier is built for, restated on the reference side: each changes at least one output of this scene
    k = 2
    others_wrong = list(range(5))                                          # `jj` instead of `jj < k ? jj : jj + 1`
    good = [j for j in range(6) if j != k]
    assert others_wrong != good and not np.array_equal(Z[:, others_wrong], Z[:, good])
    # the bound is a real assertion
    try:
        ac.ref_apply(X * 2 ** 20, Z, w)
    except AssertionError as e:
        assert 'representability' in str(e)
    else:
        raise AssertionError('the bound did not fire')
    Xd, wl, wg = ac.onchip_scene(5, 2, 3, 2, 4, 33, dither=True)
    z, yf = ac.ref_onchip(Xd, wl, wg, q=16)
    assert np.array_equal(z * 8, np.round(z.real * 8) + 1j * np.round(z.imag * 8)) and np.abs(Xd.real * 4 % 2).min() == 1
    # the layout helpers are the covariance tier's (tests/test_cov_routes_cpu.py holds them against the header)
    assert ac.z_to_blocks is cc.z_to_blocks


def test_restatement_rounds_and_the_reference_does_not():
    """The bar of the inverse-transform tier on a fixed seed: the float32 restatement sits at float32 rounding level from the float64
    oracle in every hop segment, the oracle reproduces a float64 overlap-add written out here, and one hop segment scaled wrongly at a
    run boundary -- or dropped, or a wrong last-segment factor -- is far outside the bar while a whole-signal 2-norm at 1e-4 passes."""
    for n_fft, L in ((512, 17 * 256 + 100), (1024, 6 * 512), (512, 77)):
        hop = n_fft // 2
        T = 1 + L // hop
        yf = ac.spectra(np.random.default_rng(7), (2, 2, T, hop + 1), dither=True)
        ref = ac.istft_f64(yf, L, n_fft)
        ac.assert_segments_comparable(ref, hop)
        got = ac.istft_f32(yf, L, n_fft)
        assert ref.dtype == np.float64 and got.dtype == np.float32 and got.shape == ref.shape == (2, 2, L)
        q = ac.segment_quantity(got, ref, hop)
        assert q.shape == (2, 2, -(-L // hop)) and 2e-8 < q.min() and q.max() < 2e-6, (q.min(), q.max())
        assert ac.segment_quantity(ref, ref, hop).max() == 0
        if T > 4:
            bad = ref.copy()
            bad[1, 0, 5 * hop:6 * hop] *= 1 + 1e-4                         # one segment of one signal, 1e-4 off
            qb = ac.segment_quantity(bad, ref, hop)
            assert qb[1, 0, 5] > 10 * ac.BAR_FACTOR * q[1, 0, 5] and (np.delete(qb.reshape(4, -1), 5, axis=1)[2] == 0).all()
            assert np.linalg.norm(bad - ref) / np.linalg.norm(ref) < 1e-4
    # the last-segment factor applied one segment early (seg + 2 >= T): that segment is divided by w_hi^2 instead of the full window sum
    n_fft, hop, L = 512, 256, 9 * 256 + 100
    T = 1 + L // hop
    yf = ac.spectra(np.random.default_rng(8), (1, 1, T, 257), dither=True)
    ref, got = ac.istft_f64(yf, L, n_fft), ac.istft_f32(yf, L, n_fft)
    win = ac.so.hann_periodic(n_fft)
    early = ref.copy()
    early[0, 0, (T - 2) * hop:(T - 1) * hop] *= (win[hop:] ** 2 + win[:hop] ** 2) / np.maximum(win[hop:] ** 2, 1e-300)
    q, qe = ac.segment_quantity(got, ref, hop), ac.segment_quantity(early, ref, hop)
    assert qe[0, 0, T - 2] > 1e3 * ac.BAR_FACTOR * q[0, 0, T - 2] and qe[0, 0, T - 1] == 0
    # per-room lengths: a room is processed as if alone at its own length
    yf2 = ac.spectra(np.random.default_rng(9), (2, 1, T, 257), dither=True)
    yf2[1, :, 4:] = 0
    both = ac.room_wise(ac.istft_f64, yf2, L, n_fft, [L, 3 * 256 + 17])
    assert np.array_equal(both[0], ac.istft_f64(yf2[0], L, n_fft)) and not both[1, :, 3 * 256 + 17:].any()
    assert np.array_equal(both[1, :, :3 * 256 + 17], ac.istft_f64(yf2[1, :, :4], 3 * 256 + 17, n_fft))
    assert ac.length_of(3, 0, 256) == 768 and ac.length_of(3, 10, 256) == 522


def test_committed_ratios_are_inside_the_bar():
    import json
    rec = json.loads(_read(REPO, 'profiles', 'apply_routes_errors.json'))
    fams = {'k_istft<512>', 'k_istft<1024>', 'k_step2_apply_istft<512>', 'k_apply_istft_wide<512>', 'k_apply_istft_wide<1024>'}
    assert set(rec['ratio_to_float32_restatement']) == fams and rec['bar_factor'] == ac.BAR_FACTOR
    for fam, row in rec['ratio_to_float32_restatement'].items():
        assert 0 < row['median'] <= row['worst'] <= ac.BAR_FACTOR and row['segments'] > 100, (fam, row)
