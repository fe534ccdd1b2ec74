"""BASELINE.json configs[3] plumbing: CRNN masks (PyTorch-ROCm) in the loop around the HIP kernels."""
import numpy as np
import pytest

import parity_checks as pc
from disco_amd import _lib, synth
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu

# the north star's bar; the MWF is fed the SAME masks on both sides, so nothing network-specific enters the comparison
CRNN_TOL = float(__import__('os').environ.get('DISCO_CRNN_TOL', '1e-4'))


def _rand_model(n_ch, seed, device):
    import torch
    from torch import nn
    from disco_amd.dnn.crnn import build_crnn
    torch.manual_seed(seed)
    m = build_crnn(n_ch=n_ch)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
    with torch.no_grad():                     # spread the (random) masks over (0, 1): masks stuck near 0.5 would make
        m.ff.layers[0].weight.mul_(40.0)      # Rss ~ Rnn, a degenerate eigenproblem no implementation can reproduce tightly
    return m.to(device).eval()


@pytest.mark.parametrize('K,M,two_models', [(3, 2, True), (4, 4, False), (1, 4, True)])
def test_crnn_in_loop_vs_oracle(K, M, two_models):
    import torch
    from disco_amd.dnn.inloop import tango_enhance_dnn
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    R, L = 2, 24000
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=_lib.load())
    dev = torch.device('cuda', 0)
    model_z = _rand_model(1, 1, dev)
    model_w = _rand_model(K, 2, dev) if (two_models and K > 1) else None
    out, mz, mw = tango_enhance_dnn(eng, torch.from_numpy(y).to(dev), model_z, model_w, want_masks=True)
    out, mz, mw = out.cpu().numpy(), mz.cpu().numpy(), mw.cpu().numpy()
    assert np.all((mz >= 0) & (mz <= 1)) and np.all(np.isfinite(out))
    cpu_z = _rand_model(1, 1, 'cpu').double()
    for r in range(R):
        # 1) the MWF around the masks: feed the SAME masks to the float64 oracle
        masks = ([mz[r, k].T.astype(np.float64) for k in range(K)], [mw[r, k].T.astype(np.float64) for k in range(K)])
        o = to.offline_tango_vec(y[r], s[r], n[r], masks=masks, precision='f64', solver='eigh')
        for k in range(K):
            ref = so.istft(o['yf'][k], L, work_dtype=np.float64)
            assert pc.relerr(out[r, k], ref) < CRNN_TOL, (r, k, pc.relerr(out[r, k], ref))
        # 2) the step-1 masks themselves: the same network in float64 on the oracle's |Y_ref|
        mag = np.stack([np.abs(o['Y'][k][0]).T for k in range(K)])[:, None]            # (K, 1, T, F)
        ref_mz = cpu_z.predict_masks(torch.from_numpy(mag)).numpy()
        assert np.abs(ref_mz - mz[r]).max() < 2e-4
        # 3) the step-2 masks: channel order [|Y_k|, |z_j| j != k] (tango.py:158-186, 391)
        if model_w is not None:
            cpu_w = _rand_model(K, 2, 'cpu').double()
            zmag = [np.abs(o['z_y'][j]).T for j in range(K)]
            inp = np.stack([np.stack([np.abs(o['Y'][k][0]).T] + [zmag[j] for j in range(K) if j != k]) for k in range(K)])
            ref_mw = cpu_w.predict_masks(torch.from_numpy(inp)).numpy()
            assert np.abs(ref_mw - mw[r]).max() < 2e-3          # |z| carries the (bounded) step-1 mask differences
        else:
            assert np.array_equal(mw, mz)                        # tango.py:388-389


@pytest.mark.parametrize('two_models', [True, False])
def test_offline_tango_with_crnn_masks(two_models):
    """The reference call surface with vads='crnn' and models in `mods` (tango.py:209-215, 387-394): the masks it returns are
    the networks' predictions, and every other output equals the float64 oracle fed with those masks."""
    import torch
    from disco_amd.speech_enhancement.tango import offline_tango
    from oracle import tango_oracle as to
    K, M, L = 3, 2, 20000
    y, s, n, _ = synth.make_room_numpy(12, K=K, M=M, L=L)
    dev = torch.device('cuda', 0)
    model_z = _rand_model(1, 1, dev)
    model_w = _rand_model(K, 2, dev) if two_models else None
    res = offline_tango(list(y), list(s), list(n), vads=['crnn', 'crnn'], mods=[model_z, model_w])
    names = ['yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w']
    mz, mw = res[7], res[8]
    o = to.offline_tango_vec(y, s, n, masks=([m.astype(np.float64) for m in mz], [m.astype(np.float64) for m in mw]),
                             precision='f64', solver='eigh')
    ref = to.as_reference_tuple(o)
    for nm, got, want in zip(names[:7], res[:7], ref[:7]):
        for k in range(K):
            assert pc.relerr(got[k], want[k]) < CRNN_TOL, (nm, k, pc.relerr(got[k], want[k]))
    cpu_z = _rand_model(1, 1, 'cpu').double()
    mag = np.stack([np.abs(o['Y'][k][0]).T for k in range(K)])[:, None]
    ref_mz = cpu_z.predict_masks(torch.from_numpy(mag)).numpy()
    assert max(np.abs(ref_mz[k].T - mz[k]).max() for k in range(K)) < 2e-4
    if two_models:
        cpu_w = _rand_model(K, 2, 'cpu').double()
        zmag = [np.abs(o['z_y'][j]).T for j in range(K)]
        inp = np.stack([np.stack([np.abs(o['Y'][k][0]).T] + [zmag[j] for j in range(K) if j != k]) for k in range(K)])
        ref_mw = cpu_w.predict_masks(torch.from_numpy(inp)).numpy()
        assert max(np.abs(ref_mw[k].T - mw[k]).max() for k in range(K)) < 2e-3
    else:
        assert all(np.array_equal(mw[k], mz[k]) for k in range(K))


def test_crnn_features_vs_torch():
    """The networks' input features in one pass (disco_crnn_features) against torch's abs / index copies / clamp / pad."""
    import torch
    torch.cuda.set_device(0)
    print(pc.check_crnn_features(_lib.load(), 'cuda:0'))
    print(pc.check_crnn_features(_lib.load(), 'cuda:0', R=3, K=4, M=4, T=40, F=257))


def test_conv3x3_pool4_vs_torch():
    """The first block of the convolutional stack in one pass (disco_conv3x3_pool4) against torch's conv2d + max_pool2d in float64."""
    import torch
    torch.cuda.set_device(0)
    print(pc.check_conv3x3_pool4(_lib.load(), 'cuda:0'))


def test_gru_gates_vs_float64():
    """The GRU step's gate arithmetic (disco_gru_gates) against float64, chained over 8 and 15 steps against torch.nn.GRU, and at
    n = 70 000 x H = 256 (more elements than one launch pass covers)."""
    import torch
    torch.cuda.set_device(0)
    print(pc.check_gru_gates(_lib.load(), 'cuda:0', chain=(4096, 256, 256), big=True))


def test_maxpool_last4_vs_torch():
    """MaxPool (1, 4) + bias (disco_maxpool_last4) against torch bit for bit, non-finite windows, and more than 2^28 outputs."""
    import torch
    torch.cuda.set_device(0)
    assert pc.check_maxpool_last4(_lib.load(), 'cuda:0', big=True)


def test_crnn_windows_vs_strided():
    """The recurrent layer's input windows (disco_crnn_windows) against predict_masks' strided fallback, bit for bit."""
    import torch
    torch.cuda.set_device(0)
    assert pc.check_crnn_windows(_lib.load(), 'cuda:0')


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('tag,n_ch', [('sc', 1), ('mc', 4)])
@pytest.mark.parametrize('ftp', ['mid', 'last'])
def test_predict_masks_float32_vs_float64_production_shape(golden_dir, tag, n_ch, ftp, fused):
    """predict_masks in float32 -- every HIP helper of the network on its path -- against the same trained network in float64 on the
    same GPU (all helpers are gated on float32: that run is plain torch), at a shape past every single-pass launch: 300 signals (chunks
    of 256 + 44) of 300 frames, so 76 800 GRU rows per step."""
    import copy
    import os
    import torch
    from disco_amd.dnn.crnn import build_crnn
    gold = np.load(os.path.join(golden_dir, 'crnn_ref.npz'))
    sd = {k[len(tag) + 4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(f'{tag}_sd_')}
    dev = torch.device('cuda', 0)
    model = build_crnn(n_ch=n_ch, state_dict=sd).to(dev).eval()
    model.fused_first_block = fused
    ref_model = copy.deepcopy(model).double()
    B, T, F = 300, 300, 257
    g = torch.Generator(device=dev).manual_seed(n_ch * 10 + fused)
    level = torch.exp(2.0 * torch.randn((B, n_ch, T, 1), device=dev, generator=g))               # loud and near-silent frames
    mag = torch.randn((B, n_ch, T, F), device=dev, generator=g).abs() * level
    mask = model.predict_masks(mag, frame_to_pred=ftp)
    want = ref_model.predict_masks(mag.double(), frame_to_pred=ftp)
    assert mask.dtype == torch.float32 and mask.shape == (B, T, F)
    err = float((mask.double() - want).abs().max())
    print(tag, ftp, 'fused' if fused else 'library', 'max |mask32 - mask64|', err)
    assert err < 2e-5, err


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('tag,n_ch', [('sc', 1), ('mc', 4)])
@pytest.mark.parametrize('ftp,nt', [('mid', None), ('last', None), ('mid', 'scale_to_unit_norm'), ('mid', 'scale_to_1'), ('last', 'center_and_scale')])
def test_predict_masks_on_gpu_vs_reference_fixture(golden_dir, tag, n_ch, ftp, nt, fused):
    """predict_masks on the MI355X -- the path with the HIP helpers disco_crnn_windows / disco_gru_gates / disco_maxpool_last4 active --
    (and, `fused`, the first convolution block through disco_conv3x3_pool4 or through the library convolution + pooling pass) --
    DIRECTLY against the outputs of the reference's own model / prepare_data / reshape_mask (dnn/models/crnn.py:55-63,
    speech_enhancement/utils.py:69-138; tests/golden/crnn_ref.npz, crnn_variants_ref.npz): one link, no CPU evaluation in between
    (VERDICT round 3, item 5 of "what's missing").  2e-5 on masks in [0, 1]: float32 GEMMs / convolutions of another library."""
    import os
    import torch
    from disco_amd.dnn.crnn import build_crnn
    gold = np.load(os.path.join(golden_dir, 'crnn_ref.npz'))
    var = np.load(os.path.join(golden_dir, 'crnn_variants_ref.npz'))
    sd = {k[len(tag) + 4:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(f'{tag}_sd_')}
    dev = torch.device('cuda', 0)
    model = build_crnn(n_ch=n_ch, state_dict=sd).to(dev).eval()
    model.fused_first_block = fused             # both routes of the first block: disco_conv3x3_pool4 / library convolution + pooling pass
    chans = [np.abs(gold[f'{tag}_Y'])]
    if n_ch > 1:
        chans += [np.abs(z) for z in gold[f'{tag}_Z']]
    mag = torch.from_numpy(np.stack(chans)[None].transpose(0, 1, 3, 2).copy()).to(dev)          # (1, n_ch, T, F)
    mask = model.predict_masks(mag, frame_to_pred=ftp, norm_type=nt)
    assert mask.is_cuda
    mask = mask.cpu().numpy()[0]
    ref = gold[f'{tag}_mask'] if (ftp == 'mid' and nt is None) else var[f'{tag}_{ftp}_{nt}']    # (F, T)
    assert mask.shape == ref.T.shape
    err = float(np.abs(mask - ref.T).max())
    assert err < 2e-5, err
    print(tag, ftp, nt, 'max |mask - reference|', err)


def test_in_loop_path_on_given_saturating_masks_and_its_spectra():
    """The kernel sequence of the in-loop path (disco_stft, disco_cov_masked, pending solves, disco_step2_cov_fused, one-pass filter + iSTFT)
    on GIVEN masks with saturated bins -- what bench.py does with C4's predictions: `masks=` re-runs the sequence, `want_yf=True` hands out
    the filtered spectra of that step (their iSTFT == the one-pass kernel's output), and the room is scored without setting anything aside
    (bench.score_given_masks: unflagged bins at 1e-4, flagged bins against the reference's own solve)."""
    import os
    import sys
    import torch
    from disco_amd.dnn.inloop import tango_enhance_dnn
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    R, K, M, L = 3, 4, 4, 40000
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=_lib.load())
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(11)
    ms = [pc.saturating_masks(rng, K, eng.T, eng.F) for _ in range(R)]
    mz = torch.from_numpy(np.stack([m[0] for m in ms])).to(dev)
    mw = torch.from_numpy(np.stack([m[1] for m in ms])).to(dev)
    yt = torch.from_numpy(y).to(dev)
    out = tango_enhance_dnn(eng, yt, None, None, masks=(mz, mw))                          # the one-pass final kernel
    out2, yf = tango_enhance_dnn(eng, yt, None, None, masks=(mz, mw), want_yf=True)       # the same step, spectra written
    assert torch.isfinite(out).all() and float((out - out2).abs().max()) <= 2e-6 * float(out.abs().max())
    out, yf = out.cpu().numpy(), yf.cpu().numpy()
    for r in range(R):
        masks = ([ms[r][0][k].T.astype(np.float64) for k in range(K)], [ms[r][1][k].T.astype(np.float64) for k in range(K)])
        s0, n0 = np.zeros_like(y[r]), np.zeros_like(y[r])
        s0[:, 0], n0[:, 0] = s[r][:, 0], n[r][:, 0]
        e, info = bench.score_given_masks(y[r], s0, n0, out[r], masks, yf[r], 512)
        assert e < 1e-4 and info['flagged_by_weight'] == 7 <= info['flagged_bins'] and info['spectra_vs_timed_output'] < 1e-5, (r, e, info)
