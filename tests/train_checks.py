"""Checks of the training path shared by test_train_cpu.py (torch fall-back), test_train_emulated.py (the kernels under hipemu) and
test_gpu_train.py (the MI355X).  Kernel checks take a bound library and a device; the checks that go through the package's wrappers
(SpectraBank.gather, recon_loss_frames, CRNN.forward_train) take the device only: on 'cpu' the wrappers use the torch expressions unless
the caller has put the emulated library in disco_amd._lib._lib.

Whole-model gradient figures measured with these checks, (new route, plain float32 route), each max |grad - grad64| / max |grad64| over
the whole model at B = 6:
                             n_ch 1 'all'        n_ch 1 'mid'        n_ch 4 'all'        n_ch 4 'mid'
    CPU, torch fall-back     (2.0e-6, 2.1e-6)    (2.9e-6, 3.1e-6)    (4.7e-6, 5.0e-6)    (2.65e-5, 2.70e-5)
    hipemu kernels, CPU      (1.9e-6, 2.1e-6)    (2.6e-6, 3.1e-6)    (4.3e-6, 5.0e-6)    (2.71e-5, 2.70e-5)
    MI355X                   (3.58e-2, 3.58e-2)  (1.19e-1, 1.19e-1)  (4.85e-2, 4.85e-2)  (5.35e-2, 5.35e-2)
    MI355X, native convs     (1.1e-6, 1.3e-6)    -                   -                   (1.5e-6, 1.6e-6)
On the MI355X the two routes agree with each other to 1e-6 and sit 4 to 12 % from the float64 host gradients TOGETHER: the distance is in
what they share, the library (MIOpen) convolution / BatchNorm kernels at this batch of 6 -- with torch.backends.cudnn disabled
(`native_conv`) both routes are at 1e-6 there too.  That is why the bar is the plain route's figure on the same device and not a constant.
"""
import copy
import os

import numpy as np
import torch

from disco_amd import _lib
from disco_amd.dnn import data as D
from disco_amd.dnn import losses as L
from disco_amd.dnn import train as TR
from disco_amd.dnn.crnn import build_crnn
from disco_amd.dnn.utils import get_loss_frames, get_x_for_loss

EPS32 = float(np.finfo(np.float32).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_ref.npz')
PARTS = {'all': (3, 0, 15), 'mid': (10, 7, 1), 'last': (17, 14, 1)}        # (first input frame, first output frame, frames) of the CRNN


def golden():
    return np.load(GOLDEN)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _sync(dev):
    if str(dev).startswith('cuda'):
        torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- gate kernels ---------------------------------------------------------------------------------------------------------------------

def _sig(a):
    return 1 / (1 + np.exp(-a))


def _backward64(d_out, d_carry, saved, h_prev, H, mag=False):
    """The issue's formulas in float64 from the float32 operands; mag: the same with every difference replaced by the sum of magnitudes, the
    scale against which float32 rounding of the chain is measured."""
    a = np.abs if mag else (lambda v: v)
    s = 1.0 if mag else -1.0
    r, z, c, ghn = (a(saved[:, i * H:(i + 1) * H].astype(np.float64)) for i in range(4))
    d = a(0 if d_out is None else d_out.astype(np.float64)) + a(0 if d_carry is None else d_carry.astype(np.float64))
    hp = a(np.zeros_like(r) if h_prev is None else h_prev.astype(np.float64))
    dn = d * (1 + s * z)
    dz = d * (hp + s * c)
    da_n = dn * (1 + s * c * c)
    da_z = dz * z * (1 + s * z)
    da_r = da_n * ghn * r * (1 + s * r)
    return np.concatenate((da_r, da_z, da_n), 1), np.concatenate((da_r, da_z, da_n * r), 1), d * z


def check_gates(lib, dev, n, H, later, misalign=False):
    """disco_gru_gates_train against disco_gru_gates (bits of h_out) and float64 (saved); disco_gru_gates_backward against float64, with
    strided d_out and d_gi, and with d_out / d_carry absent.  later: a step with gh and h_prev; else the first step (both NULL).
    misalign: gi and d_gi start one float past a 16-byte boundary, which takes a multiple-of-4 H off the 16-byte route."""
    rng = np.random.default_rng(100 * H + later)
    off = 1 if misalign else 0
    gi_all = _dev(rng.standard_normal(n * 9 * H + off).astype(np.float32), dev)[off:].view(n, 3, 3 * H)
    gi = gi_all[:, 1]                                                   # rows at stride 9H
    gh = _dev(rng.standard_normal((n, 3 * H)).astype(np.float32), dev) if later else None
    bias = _dev(rng.standard_normal(3 * H).astype(np.float32), dev)
    hp = _dev(rng.standard_normal((n, H)).astype(np.float32), dev) if later else None
    h_ref = torch.full((n, H), -9.0, dtype=torch.float32, device=dev)
    h_out = torch.full((n, H), -8.0, dtype=torch.float32, device=dev)
    saved = torch.full((n, 4 * H), -7.0, dtype=torch.float32, device=dev)
    assert lib.disco_gru_gates(None, gi.data_ptr(), gi.stride(0), _p(gh), bias.data_ptr(), _p(hp), h_ref.data_ptr(), n, H, None) == 0
    assert lib.disco_gru_gates_train(None, gi.data_ptr(), gi.stride(0), _p(gh), bias.data_ptr(), _p(hp), h_out.data_ptr(), saved.data_ptr(), n, H,
                                     None) == 0
    _sync(dev)
    assert torch.equal(_bits(h_ref), _bits(h_out)), 'h_out differs from disco_gru_gates in its bits'
    g64 = gi.cpu().numpy().astype(np.float64)
    q64 = (gh.cpu().numpy() if later else np.broadcast_to(bias.cpu().numpy(), (n, 3 * H))).astype(np.float64)
    r = _sig(g64[:, :H] + q64[:, :H])
    z = _sig(g64[:, H:2 * H] + q64[:, H:2 * H])
    c = np.tanh(g64[:, 2 * H:] + r * q64[:, 2 * H:])
    sv = saved.cpu().numpy()
    # r, z, c lie in [-1, 1]; pre-activations here stay below ~8 in magnitude: their float32 sum is off by <= 8 eps / 2, the sigmoid's slope is
    # <= 1/4 and tanh's <= 1, expf / tanhf / the division add a few ulp of a value <= 1, and c inherits |gh_n| x the error of r: 16 eps covers it
    tol = 16 * EPS32
    worst = max(float(np.abs(sv[:, :H] - r).max()), float(np.abs(sv[:, H:2 * H] - z).max()), float(np.abs(sv[:, 2 * H:3 * H] - c).max()))
    assert worst <= tol, (worst, tol)
    assert np.array_equal(sv[:, 3 * H:], q64[:, 2 * H:].astype(np.float32)), 'gh_n is a copy'
    h64 = (1 - z) * c + z * (hp.cpu().numpy().astype(np.float64) if later else 0)
    assert float(np.abs(h_out.cpu().numpy() - h64).max()) <= 2 * tol
    # backward
    d_out_all = _dev(rng.standard_normal((n, 2, H)).astype(np.float32), dev)
    d_carry = _dev(rng.standard_normal((n, H)).astype(np.float32), dev)
    figs = []
    for d_out, dc in ((d_out_all[:, 1], d_carry), (None, d_carry), (d_out_all[:, 1], None)):
        d_gi_all = torch.full((n * 9 * H + off,), -5.0, dtype=torch.float32, device=dev)[off:].view(n, 3, 3 * H)
        d_gi = d_gi_all[:, 2]
        d_gh = torch.full((n, 3 * H), -4.0, dtype=torch.float32, device=dev)
        d_h = torch.full((n, H), -3.0, dtype=torch.float32, device=dev)
        rc = lib.disco_gru_gates_backward(None, _p(d_out), 0 if d_out is None else d_out.stride(0), _p(dc), saved.data_ptr(), _p(hp), d_gi.data_ptr(),
                                          d_gi.stride(0), d_gh.data_ptr(), d_h.data_ptr(), n, H, None)
        assert rc == 0, rc
        _sync(dev)
        args = (None if d_out is None else d_out.cpu().numpy(), None if dc is None else dc.cpu().numpy(), sv, hp.cpu().numpy() if later else None, H)
        ref, mag = _backward64(*args), _backward64(*args, mag=True)
        assert bool((d_gi_all[:, :2] == -5.0).all()), 'd_gi rows of other steps were written'
        # every output is a chain of at most 7 float32 operations on the float32 operands: 8 eps of the chain's magnitude
        for got, want, scale in zip((d_gi, d_gh, d_h), ref, mag):
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            assert bool((err <= 8 * EPS32 * scale + 1e-37).all()), float((err / (scale + 1e-30)).max())
            figs.append(float((err / (scale + 1e-30)).max()) / EPS32)
    return max(figs)


def check_gate_refusals(lib, dev):
    H, n = 4, 4
    a = torch.zeros((n, 4 * H), dtype=torch.float32, device=dev)
    p = a.data_ptr()
    assert lib.disco_gru_gates_train(None, p, 11, None, p, None, p, p, n, H, None) == -1          # gi_stride < 3H
    assert lib.disco_gru_gates_train(None, p, 12, None, None, None, p, p, n, H, None) == -1        # no gh, no bias
    assert lib.disco_gru_gates_train(None, p, 12, None, p, None, p, None, n, H, None) == -1        # no saved
    assert lib.disco_gru_gates_train(None, p, 12, None, p, None, p, p, 0, H, None) == -1
    assert lib.disco_gru_gates_backward(None, None, 0, None, p, None, p, 12, p, p, n, H, None) == -1      # neither d_out nor d_carry
    assert lib.disco_gru_gates_backward(None, p, 3, None, p, None, p, 12, p, p, n, H, None) == -1         # d_out_stride < H
    assert lib.disco_gru_gates_backward(None, p, 4, None, p, None, p, 11, p, p, n, H, None) == -1         # d_gi_stride < 3H
    assert lib.disco_gru_gates_backward(None, p, 4, None, None, None, p, 12, p, p, n, H, None) == -1      # no saved
    return True


# ---- loss kernels ---------------------------------------------------------------------------------------------------------------------

def _loss64(est, y, x, ff_in):
    n_out = est.shape[1]
    e = est.astype(np.float64) - y[:, ff_in:ff_in + n_out].astype(np.float64)
    w = x[:, 0, ff_in:ff_in + n_out].astype(np.float64)
    t = (e * w) ** 2
    ok = ~np.isnan(t)
    return t, ok, e, w


def _run_loss(lib, dev, est, y, x, ff_in):
    B, n_out, F = est.shape
    C, W = x.shape[1:3]
    te, ty, tx = _dev(est, dev), _dev(y, dev), _dev(x, dev)
    sums = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.RECON_LOSS_WS_BYTES // 8, dtype=torch.float64, device=dev)
    assert lib.disco_recon_loss(None, te.data_ptr(), ty.data_ptr(), tx.data_ptr(), B, C, W, F, ff_in, n_out, sums.data_ptr(), ws.data_ptr(),
                                _lib.RECON_LOSS_WS_BYTES, None) == 0
    g = _dev(np.array([0.7], np.float32), dev)
    d_est = torch.full((B, n_out, F), -6.0, dtype=torch.float32, device=dev)
    assert lib.disco_recon_loss_grad(None, te.data_ptr(), ty.data_ptr(), tx.data_ptr(), B, C, W, F, ff_in, n_out, sums.data_ptr(), g.data_ptr(),
                                     d_est.data_ptr(), None) == 0
    _sync(dev)
    return sums.cpu().numpy(), d_est.cpu().numpy()


def check_loss(lib, dev, C, F, part, fixture=None):
    """disco_recon_loss / _grad at B = 3, W = 21: sum and count against float64 NumPy of the same expression (relative 1e-12, exact), two runs
    bit-equal, NaNs planted in est and in x drop out of the count and leave +0.0 in the gradient, the gradient within 1 ulp of the float64
    gradient rounded to float32; fixture (F = 17): the inputs and the reference's own reconstruction_loss values."""
    ff_in, ff_out, n_out = PARTS[part]
    B, W = 3, 21
    if fixture is not None:
        t = f'loss_c{C}_f{F}'
        est_all, y, x = (fixture[t + s].astype(np.float32) for s in ('_est', '_y', '_x'))
        nan_est, nan_x = fixture[t + '_nan_est'], fixture[t + '_nan_x']
    else:
        rng = np.random.default_rng(1000 * C + F)
        est_all = rng.random((B, 15, F)).astype(np.float32)
        y = rng.random((B, W, F)).astype(np.float32)
        x = (2 * rng.random((B, C, W, F))).astype(np.float32)
        nan_est, nan_x = np.array([[0, 3, 5], [2, 14, F - 1], [1, 7, 0]]), np.array([[1, 0, 10, 2], [1, 0, 3, 0], [0, 0, 17, F - 2]])
    out = {}
    for nan in (False, True):
        e_all, xx = est_all.copy(), x.copy()
        if nan:
            e_all[tuple(nan_est.T)] = np.nan
            xx[tuple(nan_x.T)] = np.nan
        est = np.ascontiguousarray(e_all[:, ff_out:ff_out + n_out])
        t64, ok, e, w = _loss64(est, y, xx, ff_in)
        sums, d_est = _run_loss(lib, dev, est, y, xx, ff_in)
        sums2, d_est2 = _run_loss(lib, dev, est, y, xx, ff_in)
        assert sums.tobytes() == sums2.tobytes() and d_est.tobytes() == d_est2.tobytes(), 'two runs differ in their bits'
        want = float(t64[ok].sum())
        assert sums[1] == ok.sum(), (sums[1], ok.sum())
        assert abs(sums[0] - want) <= 1e-12 * want, (sums[0], want)
        if nan:
            assert ok.sum() < ok.size, 'no planted NaN fell on a loss frame'
        if fixture is not None:
            ref = float(fixture[f'{t}_{part}{"_nan" if nan else ""}'])
            assert abs(sums[0] / sums[1] - ref) <= 1e-12 * ref, (sums[0] / sums[1], ref)
        g64 = np.float64(np.float32(0.7)) * 2 * e * w * w / ok.sum()
        g32 = g64.astype(np.float32)
        assert bool((d_est[~ok] == 0).all()) and not bool(np.signbit(d_est[~ok]).any()), 'gradient at a NaN term is not +0.0'
        ulp = np.spacing(np.abs(g32[ok]))
        assert bool((np.abs(d_est[ok] - g32[ok]) <= ulp).all())
        out[nan] = (float(sums[0] / sums[1]), int(sums[1]))
    assert out[True][1] < out[False][1] or part != 'all'
    return out


def check_loss_refusals(lib, dev):
    a = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = a.data_ptr()
    ok = (3, 1, 21, 17, 3, 15)
    assert lib.disco_recon_loss(None, p, p, p, *ok, p, p, 16384, None) == 0
    assert lib.disco_recon_loss(None, p, p, p, 3, 1, 21, 17, 7, 15, p, p, 16384, None) == -1       # ff_in + n_out > W
    assert lib.disco_recon_loss(None, p, p, p, 3, 1, 21, 17, -1, 15, p, p, 16384, None) == -1
    assert lib.disco_recon_loss(None, p, p, p, *ok, p, p, 15, None) == -1                          # workspace too small
    assert lib.disco_recon_loss(None, p, p, p, *ok, None, p, 16384, None) == -1
    assert lib.disco_recon_loss_grad(None, p, p, p, *ok, p, None, p, None) == -1                   # no g
    assert lib.disco_recon_loss_grad(None, p, p, p, 3, 1, 21, 17, 7, 15, p, p, p, None) == -1
    _sync(dev)
    return True


# ---- gather -----------------------------------------------------------------------------------------------------------------------------

def _fixture_bank(fx):
    return fx['bank_u8'].astype(np.float32) / 16                        # (S, N, F, T), the reference's orientation


def _gather(lib, dev, bank_tf, tab, C, W, tab_host=True, fill=-7.0):
    S, N, T, F = bank_tf.shape
    B = tab.shape[0]
    tab = np.ascontiguousarray(tab, np.int32)
    x = torch.full((B, C, W, F), fill, dtype=torch.float32, device=dev)
    y = torch.full((B, W, F), fill, dtype=torch.float32, device=dev)
    td = _dev(tab, dev)
    rc = lib.disco_train_batch(None, bank_tf.data_ptr(), S, N, T, F, td.data_ptr(), tab.ctypes.data if tab_host else None, B, C, W, x.data_ptr(),
                               y.data_ptr(), None)
    _sync(dev)
    return rc, x.cpu().numpy(), y.cpu().numpy()


def check_gather_fixture(lib, dev):
    """disco_train_batch, bit-equal to the windows the reference's get_subwindow / get_mask_frames returned for the fixture's (k, m, rows):
    m = 0, m = n_frames - W, the segment of exactly W frames and every local node are among them; no sentinel survives."""
    fx = golden()
    bank = _dev(_fixture_bank(fx).transpose(0, 1, 3, 2), dev)
    W = 21
    for tag in ('z3', 'z1'):
        tab = fx[tag + '_tab']
        C = tab.shape[1] - 3
        rc, x, y = _gather(lib, dev, bank, tab, C, W)
        assert rc == 0, rc
        want_x = (fx[tag + '_x_u8'].astype(np.float32) / 16).transpose(0, 1, 3, 2)
        want_y = (fx[tag + '_y_u8'].astype(np.float32) / 16).transpose(0, 2, 1)
        assert x.min() >= 0 and y.min() >= 0, 'a sentinel survived'
        assert np.array_equal(x, want_x) and np.array_equal(y, want_y), tag
    m, k = fx['z3_tab'][:, 1], fx['z3_tab'][:, 0]
    assert (m == 0).any() and (m == fx['n_frames'][k] - W).any() and (fx['n_frames'][k] == W).any() and set(fx['z3_local']) == {0, 1, 2, 3}
    return True


def check_gather_257_and_refusals(lib, dev):
    """F = 257 (runs that keep no 16-byte alignment), more runs than one pass of a small grid would need is not the point here: against NumPy
    indexing.  Bad host tables: DISCO_E_ARG, nothing written; the same entries on the device alone: zeros for that item, no read outside the bank."""
    rng = np.random.default_rng(9)
    S, N, T, F, W, C = 8, 2, 30, 257, 21, 1
    bank_np = rng.random((S, N, T, F)).astype(np.float32) + 1
    bank = _dev(bank_np, dev)
    tab = np.array([[0, 0, 1, 5], [1, 9, 3, 7], [1, 4, 0, 4], [0, 9, 2, 6]], np.int32)
    rc, x, y = _gather(lib, dev, bank, tab, C, W)
    assert rc == 0
    for b, (k, m, r0, r1) in enumerate(tab):
        assert np.array_equal(x[b, 0], bank_np[r0, k, m:m + W]) and np.array_equal(y[b], bank_np[r1, k, m:m + W])
    for col, val in ((1, 10), (1, -1), (0, 2), (0, -1), (2, 8), (3, -1)):               # m + W > T, m < 0, segment, signal rows
        bad = tab.copy()
        bad[2, col] = val
        rc, x, y = _gather(lib, dev, bank, bad, C, W)
        assert rc == -1 and (x == -7.0).all() and (y == -7.0).all(), (col, val, rc)
        rc, x, y = _gather(lib, dev, bank, bad, C, W, tab_host=False)
        assert rc == 0 and (x != -7.0).all() and (y != -7.0).all()
        assert (x[2] == 0).all() or (y[2] == 0).all(), (col, val)
        assert np.array_equal(x[1, 0], bank_np[3, 1, 9:30])
    return True


def check_bank_gather(dev):
    """SpectraBank.gather (the wrapper: disco_train_batch on a GPU or with the emulated library bound, torch indexing on the CPU) on the fixture,
    from complex input in the reference's orientation; a bad table raises ValueError."""
    fx = golden()
    data = _fixture_bank(fx)
    for tag, zn in (('z3', 3), ('z1', 1)):
        bank = D.SpectraBank((data * np.exp(1j * 0.3)).astype(np.complex64), n_frames=fx['n_frames'], stack_axis=2, z_nodes=zn, device=dev)
        assert bank.data.dtype == torch.float32 and tuple(bank.data.shape) == (12, 3, 40, 17)
        x, y = bank.gather(fx[tag + '_tab'])
        want_x = (fx[tag + '_x_u8'].astype(np.float32) / 16).transpose(0, 1, 3, 2)
        assert float(np.abs(x.cpu().numpy() - want_x).max()) < 1e-5           # |k / 16 e^{0.3 i}| in complex64: a rounding away from k / 16
        bad = fx[tag + '_tab'].copy()
        bad[0, 1] = 40 - 21 + 1
        try:
            bank.gather(bad)
        except ValueError:
            pass
        else:
            raise AssertionError('m + W > T was not refused')
    real = D.SpectraBank(torch.from_numpy(data), n_frames=fx['n_frames'], stack_axis=2, device=dev)
    x, y = real.gather(fx['z3_tab'])
    assert np.array_equal(x.cpu().numpy(), (fx['z3_x_u8'].astype(np.float32) / 16).transpose(0, 1, 3, 2))
    assert np.array_equal(y.cpu().numpy(), (fx['z3_y_u8'].astype(np.float32) / 16).transpose(0, 2, 1))
    return True


# ---- draws (host only) --------------------------------------------------------------------------------------------------------------------

def check_draws():
    fx = golden()
    data = _fixture_bank(fx)
    bank = D.SpectraBank(data, n_frames=fx['n_frames'], stack_axis=2)
    assert len(bank) == int(fx['len']) == int(fx['win_per_seg'].sum()) and np.array_equal(bank.windows_per_segment(), fx['win_per_seg'])
    k, m = bank.item_indices(fx['idx_item'], fx['idx_jitter'])
    assert np.array_equal(k, fx['idx_k']) and np.array_equal(m, fx['idx_m'])
    for item, jit, kk, mm in zip(fx['idx_item'], fx['idx_jitter'], fx['idx_k'], fx['idx_m']):
        assert tuple(int(v) for v in bank.item_indices(int(item), int(jit))) == (kk, mm)
    K, S = 4, 12
    for zn, C in ((3, 4), (1, 2), (0, 1)):
        b = D.SpectraBank(data, n_frames=fx['n_frames'], stack_axis=2, z_nodes=zn)
        assert b.n_ch == C
        rng = np.random.default_rng(zn)
        items = np.tile(np.arange(len(b)), 100)
        tab = b.draw_batch(items, rng)
        assert tab.dtype == np.int32 and tab.shape == (items.size, C + 3)
        local = tab[:, 2]
        assert set(local) == set(range(K)) and np.array_equal(tab[:, -1], S - K + local)
        k0, m0 = b.item_indices(items, 0)
        k7, m7 = b.item_indices(items, 7)
        assert np.array_equal(tab[:, 0], k0) and (tab[:, 1] >= m0).all() and (tab[:, 1] <= m7).all()
        assert len(set(tab[:, 1][items == 0])) == 8                                # every jitter of item 0 occurs
        if zn == 3:
            for i in range(3):
                assert np.array_equal(tab[:, 3 + i], K + np.array([np.roll(np.arange(K), K - 1 - l)[i] for l in local]))
        if zn == 1:
            z = tab[:, 3] - K
            assert (z != local).all() and (z >= 0).all() and (z < K).all()
            for l in range(K):
                assert set(z[local == l]) == set(range(K)) - {l}
    sc = D.SpectraBank(data[[0, 1, 2, 3, 8, 9, 10, 11]], n_frames=fx['n_frames'], stack_axis=0)
    assert sc.n_ch == 1 and sc.draw_batch([0, 1], np.random.default_rng(0)).shape == (2, 4)
    x, y = next(D.batches(sc, 4, np.random.default_rng(1)))
    assert tuple(x.shape) == (4, 21, 17) and tuple(y.shape) == (4, 21, 17)
    assert sum(xb.shape[0] for xb, _ in D.batches(sc, 4, np.random.default_rng(1))) == len(sc) and D.n_batches(sc, 4) == 2
    try:
        D.SpectraBank(data, stack_axis=1)
    except NotImplementedError:
        pass
    else:
        raise AssertionError('stack_axis=1 was accepted')
    return True


def check_from_files(tmp_path):
    rng = np.random.default_rng(4)
    lens = (70, 60)
    lists = [[None] * 2 for _ in range(8)]
    arrs = {}
    for i in range(8):
        for j, T in enumerate(lens):
            a = (rng.standard_normal((17, T - (i == 5))) + 1j * rng.standard_normal((17, T - (i == 5)))).astype(np.complex64)
            lists[i][j] = os.path.join(str(tmp_path), f'{i}_{j}.npy')
            np.save(lists[i][j], a)
            arrs[i, j] = a
    bank = D.SpectraBank.from_files(lists, fs=16000, hop=512, win_len=21)        # skips ceil(16000 / 512) = 32 frames
    assert (bank.S, bank.N, bank.T, bank.F) == (8, 2, 38, 17) and list(bank.n_frames) == [38, 28]
    assert np.array_equal(bank.data[3, 1, :28].numpy(), np.abs(arrs[3, 1])[:, 32:].T) and float(bank.data[3, 1, 28:].abs().max()) == 0
    assert float(bank.data[5, 0, 37].abs().max()) == 0                             # the row one frame short is zero-filled
    return True


# ---- restated helpers against the reference's records ------------------------------------------------------------------------------------------

def check_helpers():
    fx = golden()
    model = build_crnn(1)
    for part in ('all', 'mid', 'last'):
        assert tuple(get_loss_frames(21, part)) == tuple(fx[f'frames_21_{part}']) and tuple(get_loss_frames(15, part)) == tuple(fx[f'frames_15_{part}'])
        got = model.get_loss_frames(part)
        assert np.array_equal(np.array(got), fx[f'crnn_frames_{part}']), (part, got)
        assert (got[0][0], got[1][0], got[1][1] - got[1][0]) == PARTS[part]
        for dim in (3, 4):
            x = torch.from_numpy(fx[f'sel_x{dim}'])
            assert np.array_equal(get_x_for_loss(x, part, n_freq=7).numpy(), fx[f'sel{dim}_{part}_nomodel'])
            assert np.array_equal(get_x_for_loss(x, part, model=model, model_output=0, n_freq=7).numpy(), fx[f'sel{dim}_{part}_model0'])
    assert tuple(get_loss_frames(21, 5)) == tuple(fx['frames_21_int5'])
    vals = fx['cb_values']
    for tag, kw, v in (('min', dict(patience=2, mode='min'), vals), ('min_delta', dict(patience=1, mode='min', delta=0.05), vals),
                       ('max', dict(patience=2, mode='max', delta=0.01), 1 - vals)):
        cb = TR.SaveAndStop(**kw)
        rec = [[int(cb.save_model_query(a)), cb.waited, int(cb.early_stop_query())] for a in v]
        assert np.array_equal(np.array(rec), fx[f'cb_{tag}']), tag
    for C in (1, 4):                                                            # reconstruction_loss / nanmean, float64, against the reference's values
        t = f'loss_c{C}_f17'
        est, y, x = (torch.from_numpy(fx[t + s].astype(np.float64)) for s in ('_est', '_y', '_x'))
        for part, (ff_in, ff_out, n_out) in PARTS.items():
            for nan in (False, True):
                e, xx = est.clone(), x.clone()
                if nan:
                    e[tuple(fx[t + '_nan_est'].T)] = float('nan')
                    xx[tuple(fx[t + '_nan_x'].T)] = float('nan')
                got = L.reconstruction_loss(y[:, ff_in:ff_in + n_out], e[:, ff_out:ff_out + n_out], xx[:, 0, ff_in:ff_in + n_out]).item()
                ref = float(fx[f'{t}_{part}{"_nan" if nan else ""}'])
                assert abs(got - ref) <= 1e-12 * ref
    m, opt = TR.load_architecture(4)
    assert isinstance(opt, torch.optim.RMSprop) and opt.clip is False and opt.defaults['lr'] == 0.001 and m.input_shape == (4, 21, 257)
    assert set(m.state_dict()) == set(build_crnn(4).state_dict())
    return True


# ---- whole-model gradients ------------------------------------------------------------------------------------------------------------------

def _model_inputs(n_ch, dev):
    g = torch.Generator().manual_seed(5)
    x = 2 * torch.rand((6, n_ch, 21, 257), generator=g)
    y = torch.rand((6, 21, 257), generator=g)
    if n_ch == 1:
        x = x[:, 0]                                                     # (B, W, F), as the data set returns it for one channel
    return x.to(dev), y.to(dev)


def _plain_loss(model, x, y, part):
    est = model(x)
    return L.reconstruction_loss(get_x_for_loss(y, part, model=model, model_output=0), get_x_for_loss(est, part, model=model, model_output=1),
                                 get_x_for_loss(x, part, model=model, model_output=0))


def check_model_grads(dev, n_ch, part, native_conv=False):
    if native_conv:                                                   # torch's own convolution / BatchNorm / GRU kernels instead of the library's
        with torch.backends.cudnn.flags(enabled=False):
            return _check_model_grads(dev, n_ch, part)
    return _check_model_grads(dev, n_ch, part)


def _check_model_grads(dev, n_ch, part):
    """Gradients of every parameter by the new route (forward_train + recon_loss_frames) and by the plain float32 route (CRNN.forward with
    nn.GRU, the loss as a torch expression), each against a float64 copy of the model run through CRNN.forward: the measure is
    max |grad - grad64| / (largest |grad64| over the whole model) -- not per parameter: the convolution biases in front of BatchNorm have
    gradients that are zero in exact arithmetic.  The new route may be at most 3 x the plain route's figure (a different summation order in
    the GEMMs, expf / tanhf against torch's).  BatchNorm's running statistics after the call are those of the plain route."""
    torch.manual_seed(3)
    base = build_crnn(n_ch).train()
    x, y = _model_inputs(n_ch, dev)
    m64 = copy.deepcopy(base).double()                                  # the float64 reference runs on the host, whatever `dev` is
    _plain_loss(m64, x.cpu().double(), y.cpu().double(), part).backward()
    g64 = {k: p.grad.to(dev) for k, p in m64.named_parameters()}
    scale = max(float(g.abs().max()) for g in g64.values())
    m_plain = copy.deepcopy(base).to(dev)
    loss_plain = _plain_loss(m_plain, x, y, part)
    loss_plain.backward()
    m_new = copy.deepcopy(base).to(dev)
    est = m_new.forward_train(x, part)
    assert tuple(est.shape) == (6, PARTS[part][2], 257)
    loss_new = L.recon_loss_frames(est, y, x, PARTS[part][0])
    loss_new.backward()
    fig = {}
    for tag, m in (('new', m_new), ('plain', m_plain)):
        fig[tag] = max(float((p.grad.double() - g64[k]).abs().max()) for k, p in m.named_parameters()) / scale
    assert abs(loss_new.item() - loss_plain.item()) <= 16 * EPS32 * loss_plain.item()
    assert fig['new'] <= 3 * fig['plain'], fig
    for (k, a), (_, b) in zip(m_new.named_buffers(), m_plain.named_buffers()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=4 * EPS32, atol=1e-9), k
        else:
            assert torch.equal(a, b) and int(a) == 1, k               # num_batches_tracked: updated once
    return fig['new'], fig['plain']


def check_kernel_route_is_taken(dev, monkeypatch):
    """forward_train and recon_loss_frames on `dev` reach the four kernels: with the entry points knocked out of the bound library they fail
    instead of quietly computing something else."""
    lib = _lib.load()
    x, y = _model_inputs(1, dev)
    model = build_crnn(1).train().to(dev)
    for name in ('disco_gru_gates_train', 'disco_gru_gates_backward', 'disco_recon_loss', 'disco_recon_loss_grad'):
        calls = []
        real = getattr(lib, name)

        def spy(*a, _real=real, _calls=calls):
            _calls.append(1)
            return _real(*a)
        monkeypatch.setattr(lib, name, spy)
        model.zero_grad()
        L.recon_loss_frames(model.forward_train(x, 'mid'), y, x, 10).backward()
        monkeypatch.setattr(lib, name, real)
        assert calls, name
    return True


# ---- fit --------------------------------------------------------------------------------------------------------------------------------------

def check_train_steps(dev, n_ch):
    """30 steps of train_one_batch on one fixed batch of 6: no loss is NaN and the last is below half the first (the plain route reaches
    0.37 x and 0.31 x for n_ch 1 and 4 on the CPU)."""
    torch.manual_seed(3)
    model, opt = TR.load_architecture(n_ch)
    model.to(dev)
    x, y = _model_inputs(n_ch, dev)
    losses = [TR.train_one_batch(model, x, y, opt, 'all') for _ in range(30)]
    assert not np.isnan(losses).any(), losses
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    ev = TR.eval_one_batch(model, x, y, 'all')
    assert np.isfinite(ev) and not model.training
    return losses[0], losses[-1]


def check_fit(dev, tmp_path):
    """fit for 2 epochs on a bank of 3 short segments writes the two files; the checkpoint loads into build_crnn, predict_masks then runs in
    eval(); a second fit resumes from it with loss arrays of length 4."""
    g = torch.Generator().manual_seed(8)
    data = torch.rand((8, 3, 257, 40), generator=g) * 2
    data[4:] = data[4:] / 2                                              # the masks: in [0, 1]
    n_frames = (40, 30, 37)
    train_bank = D.SpectraBank(data, n_frames=n_frames, device=dev)
    val_bank = D.SpectraBank(data[:, :2], n_frames=n_frames[:2], device=dev)
    torch.manual_seed(3)
    model, opt = TR.load_architecture(1)
    save = os.path.join(str(tmp_path), 'models')
    tl, vl, name = TR.fit(model, opt, train_bank, val_bank, 2, batch_size=4, save_path=save, rng=np.random.default_rng(1), name='unit', verbose=False)
    assert len(tl) == len(vl) == 2 and np.isfinite(tl).all() and np.isfinite(vl).all() and (tl > 0).all()
    losses_pt, model_pt = os.path.join(save, 'unit_losses.pt'), os.path.join(save, 'unit_model.pt')
    assert os.path.exists(losses_pt) and os.path.exists(model_pt)
    ck = torch.load(model_pt, map_location='cpu', weights_only=False)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'train_loss', 'val_loss'}
    assert set(torch.load(losses_pt, weights_only=False)) == {'train_loss', 'val_loss'}
    net = build_crnn(1, device=dev, state_dict=ck['model_state_dict'])
    masks = net.predict_masks(data[:1, 0].transpose(1, 2)[None].to(dev))
    assert tuple(masks.shape) == (1, 40, 257) and bool(torch.isfinite(masks).all()) and float(masks.min()) >= 0 and float(masks.max()) <= 1
    model2, opt2 = TR.load_architecture(1)
    tl2, vl2, name2 = TR.fit(model2, opt2, train_bank, val_bank, 2, batch_size=4, save_path=save, state_dicts=model_pt, rng=np.random.default_rng(2),
                             verbose=False)
    assert name2 == 'unit_retrain' and len(tl2) == len(vl2) == 4 and np.array_equal(tl2[:2], tl) and (tl2[2:] > 0).all()
    assert os.path.exists(os.path.join(save, 'unit_retrain_losses.pt'))
    return tl2
