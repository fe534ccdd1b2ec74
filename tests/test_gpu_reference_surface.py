"""The reference's Python call surface re-implemented on the HIP engine: offline_tango, intern_filter,
tf_mask, my_stft / my_istft -- checked against the reference's OWN outputs (tests/golden) and the oracle."""
import os

import numpy as np
import pytest

from oracle import mwf_oracle as mo
from oracle import stft_oracle as so
from oracle import tango_oracle as to

pytestmark = pytest.mark.gpu


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def test_offline_tango_signature_and_oracle_parity():
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango
    y, s, n, _ = synth.make_room_numpy(5, K=3, M=2, L=24000)
    res = offline_tango(list(y), list(s), list(n), vads=['irm1', 'irm1'], mods=[None, None])
    assert len(res) == 9 and all(len(r) == 3 for r in res)
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    ref = to.as_reference_tuple(o)
    names = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']
    for nm, got, want in zip(names, res, ref):
        for k in range(3):
            assert got[k].shape == want[k].shape == (257, 94)
            tol = 2e-5 if 'mask' in nm else 1e-4
            assert relerr(got[k], want[k]) < tol, (nm, k, relerr(got[k], want[k]))


def test_offline_tango_mask_for_z_none():
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango
    y, s, n, _ = synth.make_room_numpy(6, K=2, M=2, L=20000)
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mask_for_z=None)
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], mask_for_z=None, precision='f64', solver='eigh')
    for k in range(2):
        assert relerr(res[0][k], o['yf'][k]) < 1e-4


@pytest.mark.parametrize('mode', ['distant', 'compressed', 'use_oracle_refs', 'use_oracle_zs', 'previous'])
def test_offline_tango_mask_for_z_modes(mode, golden_dir):
    """Sender-side mask_for_z variants: vs the float64 oracle on a synthetic room (1e-4) and vs the reference's own
    outputs on the golden scene."""
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango
    y, s, n, _ = synth.make_room_numpy(8, K=3, M=2, L=20000)
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mask_for_z=mode)
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], mask_for_z=mode, precision='f64', solver='eigh')
    for k in range(3):
        for i, nm in enumerate(['yf', 'sf', 'nf']):
            assert relerr(res[i][k], o[nm][k]) < 1e-4, (mode, nm, k)
    g = np.load(os.path.join(golden_dir, 'tango_ref_modes_k2m2.npz'))
    yg = [g['y0'], g['y1']]
    sg = [g['s0'], g['s1']]
    ng = [g['n0'], g['n1']]
    res = offline_tango(yg, sg, ng, vads=['irm1', 'irm1'], mask_for_z=mode)
    for k in range(2):
        assert relerr(res[0][k], g[f'{mode}_yf{k}']) < 1e-2


def test_get_z_signals_variant():
    from disco_amd import synth
    from disco_amd.speech_enhancement.get_z_signals import offline_tango
    y, s, n, _ = synth.make_room_numpy(7, K=2, M=2, L=12000)
    z_y, z_s, z_n, zn, masks_z = offline_tango(y, s, n, vads=['irm1', 'irm1'])
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    assert relerr(z_y[1], o['z_y'][1]) < 1e-4 and relerr(zn[0], o['zn'][0]) < 1e-4


def test_offline_tango_vs_reference_golden(golden_dir):
    """Against the reference's own offline_tango output (badly conditioned toy scene: see test_gpu_parity)."""
    from disco_amd.speech_enhancement.tango import offline_tango
    g = np.load(os.path.join(golden_dir, 'tango_ref_k2m2.npz'))
    y = [g['y0'], g['y1']]
    s = [g['s0'], g['s1']]
    n = [g['n0'], g['n1']]
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mods=[None, None])
    for i, nm in enumerate(['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn']):
        for k in range(2):
            assert relerr(res[i][k], g[f'{nm}{k}']) < 1e-2, (nm, k)
    for k in range(2):
        assert np.abs(res[7][k] - g[f'masks_z{k}']).max() < 1e-3


@pytest.mark.parametrize('mode', ['local', None, 'distant', 'use_oracle_zs'])
def test_offline_tango_ragged_nodes(golden_dir, mode):
    """Nodes with different channel counts (3, 2, 2), as the reference allows: vs the reference's own outputs on the ragged
    golden scene (mode 'local') and vs the float64 oracle on a well-conditioned ragged room (every mode)."""
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango
    names = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']
    y4, s4, n4, _ = synth.make_room_numpy(9, K=3, M=4, L=20000)
    Mk = (4, 2, 3)
    y = [y4[k, :Mk[k]] for k in range(3)]
    s = [s4[k, :Mk[k]] for k in range(3)]
    n = [n4[k, :Mk[k]] for k in range(3)]
    res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mask_for_z=mode)
    o = to.as_reference_tuple(to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], mask_for_z=mode, precision='f64', solver='eigh'))
    for nm, got, want in zip(names, res, o):
        for k in range(3):
            tol = 2e-5 if 'mask' in nm else 1e-4
            assert relerr(got[k], want[k]) < tol, (mode, nm, k, relerr(got[k], want[k]))
    if mode == 'local':
        g = np.load(os.path.join(golden_dir, 'tango_ref_k3ragged.npz'))
        K = int(g['K'])
        res = offline_tango([g[f'y{k}'] for k in range(K)], [g[f's{k}'] for k in range(K)], [g[f'n{k}'] for k in range(K)],
                            vads=['irm1', 'irm1'], mods=[None, None])
        for i, nm in enumerate(names[:7]):
            for k in range(K):
                assert res[i][k].shape == g[f'{nm}{k}'].shape
                assert relerr(res[i][k], g[f'{nm}{k}']) < 2e-2, (nm, k, relerr(res[i][k], g[f'{nm}{k}']))


def test_offline_tango_ivad(golden_dir):
    """vads = 'ivad' (frame VAD of the target tiled over frequency) against the reference's own offline_tango outputs."""
    from disco_amd.speech_enhancement.tango import offline_tango
    g = np.load(os.path.join(golden_dir, 'ivad_ref.npz'))
    K = int(g['K'])
    y, s, n = ([g[f'{c}{k}'] for k in range(K)] for c in 'ysn')
    res = offline_tango(y, s, n, vads=['ivad', 'ivad'], mods=[None, None])
    names = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']
    for i, nm in enumerate(names):
        for k in range(K):
            if 'mask' in nm:
                assert np.array_equal(res[i][k], g[f'{nm}{k}']), (nm, k)
            else:
                assert relerr(res[i][k], g[f'{nm}{k}']) < 1e-3, (nm, k, relerr(res[i][k], g[f'{nm}{k}']))


def test_offline_tango_errors():
    from disco_amd.speech_enhancement.tango import offline_tango
    y = np.zeros((2, 2, 4096), np.float32)
    with pytest.raises(ValueError):
        offline_tango(y, y, y, vads=['xyz1', 'irm1'])
    with pytest.raises(NotImplementedError):
        offline_tango(y, y, y, vads=['irm1', 'irm1'], mask_for_z='use_oracle_sigs')       # broken in the reference itself


def test_intern_filter_vs_reference_golden(golden_dir):
    from disco_amd.se_utils.internal_formulas import intern_filter
    g = np.load(os.path.join(golden_dir, 'intern_filter_ref.npz'))
    seen = set()
    for i in range(int(g['n_cases'])):
        typ = str(g[f'c{i}_type'])
        seen.add(typ)
        if typ == 'gevd':
            w, (t1, si) = intern_filter(g[f'c{i}_Rxx'], g[f'c{i}_Rnn'], mu=1, type='gevd', rank=1)
        else:                                                   # 'r1-mwf' (the function's default type) and 'mwf'
            w, (t1, si) = intern_filter(g[f'c{i}_Rxx'], g[f'c{i}_Rnn'], mu=1, type=typ)
        assert w.dtype == np.complex128
        assert relerr(w, g[f'c{i}_w']) < 2e-4 and relerr(t1, g[f'c{i}_t1']) < 2e-4, (i, typ)
        # (t1, sort_index) unpacked and INDEXED, as a caller of internal_formulas.py:81 may: a permutation of range(P) like the reference's c*_sort
        # for 'gevd' (np.argsort's dtype; the values refer to the solver's own eigenvalue order -- see the shim's docstring), None otherwise
        ref_si = g[f'c{i}_sort']
        if typ == 'gevd':
            P = g[f'c{i}_Rxx'].shape[0]
            assert si.dtype == ref_si.dtype == np.int64 and si.shape == ref_si.shape == (P,)
            assert sorted(si.tolist()) == sorted(ref_si.tolist()) == list(range(P))
            assert np.arange(10 * P).reshape(P, 10)[si[::-1]].shape == (P, 10) and int(si[::-1][0]) in range(P)
        else:
            assert si is None and ref_si == -1
    assert seen == {'gevd', 'r1-mwf', 'mwf'}
    w_default, _ = intern_filter(g['c0_Rxx'], g['c0_Rnn'])      # defaults: type='r1-mwf', rank='Full' (unused by that branch)
    assert np.all(np.isfinite(w_default))
    R = np.eye(3, dtype=np.complex64)
    with pytest.raises(AttributeError):
        intern_filter(R, R, type='nope')
    with pytest.raises(TypeError):
        intern_filter(R, R + 0.1, type='gevd')


@pytest.mark.parametrize('typ', ['gevd', 'r1-mwf'])
def test_intern_filter_on_speech_minus_noise(typ):
    """intern_filter(Ryy - Rnn, Rnn, ...), the way a drop-in caller passes the speech statistics: an indefinite Rxx whose top
    generalized eigenvalue is small and positive while the dominant one is negative (noise over-estimated in most directions)."""
    from disco_amd.se_utils.internal_formulas import intern_filter
    rng = np.random.default_rng(37)
    for P in (2, 4, 7, 15):
        for trial in range(3):
            A = rng.standard_normal((P, P)) + 1j * rng.standard_normal((P, P))
            Rnn = A @ A.conj().T / P + 0.5 * np.eye(P)
            L = np.linalg.cholesky(Rnn)
            V, _ = np.linalg.qr(rng.standard_normal((P, P)) + 1j * rng.standard_normal((P, P)))
            lam = np.concatenate([[1.5], rng.uniform(0.05, 0.9, P - 1)])          # generalized spectrum of (Ryy, Rnn)
            Ryy = L @ (V * lam) @ V.conj().T @ L.conj().T
            Rxx = (Ryy - Rnn).astype(np.complex64)
            Rn = Rnn.astype(np.complex64)
            assert np.linalg.eigvalsh(Rxx.astype(np.complex128)).min() < 0
            kw = dict(type='gevd', rank=1) if typ == 'gevd' else dict(type=typ)
            w, (t1, _) = intern_filter(Rxx, Rn, mu=1, **kw)
            wr, (t1r, _) = mo.intern_filter(Rxx.astype(np.complex128), Rn.astype(np.complex128), mu=1, **kw)
            assert relerr(w, wr) < 2e-5, (P, trial, relerr(w, wr))
            if typ == 'gevd':
                assert relerr(t1, t1r) < 2e-5, (P, trial, relerr(t1, t1r))


def test_tf_mask_vs_reference_golden(golden_dir):
    from disco_amd.dnn.utils import tf_mask
    g = np.load(os.path.join(golden_dir, 'tf_mask_ref.npz'))
    for typ in ('irm1', 'irm2', 'iam1', 'iam2', 'ibm1'):
        m = tf_mask(g['S'], g['N'], type=typ)
        ref = g[typ]
        ok = np.isfinite(ref)
        if typ.startswith('ibm'):
            assert m.dtype == bool and np.mean(m != ref) < 1e-2
        else:
            assert np.abs(m[ok] - ref[ok]).max() < 1e-5 * (1 + np.abs(ref[ok]).max())
    with pytest.raises(ValueError):
        tf_mask(g['S'], g['N'], type='xyz1')
    with pytest.raises(AssertionError):
        tf_mask(g['S'], g['N'][:-1], type='irm1')


def test_my_stft_istft():
    from disco_amd.math_utils import my_istft, my_stft
    rng = np.random.default_rng(0)
    x = rng.standard_normal(16000).astype(np.float32)
    X = my_stft(x)
    ref = so.stft(x, out_dtype=np.complex128)
    assert X.shape == ref.shape == (257, 63) and X.dtype == np.complex64
    assert np.abs(X - ref).max() / np.abs(ref).max() < 2e-6
    xr = my_istft(X, 16000)
    assert xr.shape == (16000,) and np.abs(xr - x).max() < 2e-5


@pytest.mark.parametrize('idx', (0, 2))
def test_reference_run_scenes_per_bin_1e4(golden_dir, idx):
    """The reference's OWN offline_tango outputs on the long scenes of tests/golden/tango_ref_scenes.npz (fixed consecutive seeds, 201
    frames; tests/golden/make_golden_scenes.py) against the Python call surface DIRECTLY at the north star's 1e-4, per (node, bin), on
    every bin whose sensitivity the fixture's cut keeps -- no oracle in between, no seed chosen."""
    from disco_amd.speech_enhancement.tango import offline_tango
    import parity_checks as pc
    print(pc.check_reference_surface_scene_per_bin(offline_tango, golden_dir, idx))


@pytest.mark.parametrize('name', ('c3', 'c2'))
def test_baseline_shapes_surface_vs_reference(golden_dir, name):
    """offline_tango (the reference's signature) on a C3-shaped and a C2-shaped room at full length against the REFERENCE'S OWN outputs
    (tests/golden/tango_ref_baseline_shapes.npz): whole signals at 1e-4, nothing excluded."""
    from disco_amd.speech_enhancement.tango import offline_tango
    import parity_checks as pc
    print(name, pc.check_baseline_shape_surface(offline_tango, golden_dir, name))
