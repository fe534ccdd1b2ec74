"""CRNN mask estimator of DISCO, PyTorch-ROCm -- the one part of the path the north star keeps in
PyTorch.  Architecture and `state_dict` key names follow the reference so that reference-trained checkpoints load:
    disco_theque/dnn/models/crnn.py:9-63        CRNN  (3 x [Conv2d 3x3 -> BatchNorm2d -> MaxPool (1,4)] -> GRU-256 -> Linear-257 -> sigmoid)
    disco_theque/dnn/models/nn_structures.py    CNN2d / RNN / FF bricks   (key prefixes `cnn.model.*`, `rnn.model.0.rnn_layer.*`, `ff.layers.0.*`)
    disco_theque/speech_enhancement/tango.py:114-139  load_models: CRNN((n_ch, 21, 257), (32,64,64), 3x3, pool (1,4), GRU [256], FF 257, padding (0,1))
    disco_theque/speech_enhancement/utils.py:69-138   prepare_data: clip |STFT| to [1e-6, 1e3], zero-pad 10+10 frames, 21-frame windows, hop 1
    disco_theque/speech_enhancement/tango.py:228-240  reshape_mask('mid'): output frame 7 of the 15 the network returns

Two evaluation paths with identical results:
  * `forward(windows)`      -- the reference's: one (n_ch, 21, 257) window per output frame.
  * `predict_masks(mag)`    -- what the engine uses: the convolutional stack has no padding along time and pools along
    frequency only, so it is run ONCE over the whole zero-padded sequence and the 15-frame feature windows are slices of
    that; the reference's `.view` (which re-interprets the (64, 15, 4) block as (15, 256) WITHOUT a transpose,
    crnn.py:59) is reproduced on the slices; only the 8 GRU steps that reach output frame 7 are run.
"""
import functools

import numpy as np
import torch
from torch import nn

STFT_MIN, STFT_MAX = 1e-6, 1e3          # speech_enhancement/utils.py:7
WIN_LEN = 21                            # tango.py:34
PRED_FRAME = 'mid'                      # tango.py:35


def _gru_gates_hip(g, gh, b_hh, h, H):
    """One GRU step's gate arithmetic on the GPU through libdisco_hip.so (disco_gru_gates): g (n, 3H) strided rows of the
    input projection, gh (n, 3H) contiguous or None (first step), h (n, H) or None -> new h (n, H)."""
    from .. import _lib
    lib = _lib.load()
    n = g.shape[0]
    assert g.stride(1) == 1 and (gh is None or gh.is_contiguous()) and (h is None or h.is_contiguous())
    out = torch.empty((n, H), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        rc = lib.disco_gru_gates(None, g.data_ptr(), g.stride(0), None if gh is None else gh.data_ptr(), b_hh.data_ptr(),
                                 None if h is None else h.data_ptr(), out.data_ptr(), n, H, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_gru_gates failed ({rc})')
    return out


def _maxpool4_hip(x, bias):
    """MaxPool2d((1, 4)) of a (B, C, T, F) map plus the convolution's per-channel bias, on the GPU through libdisco_hip.so
    (torch's generic pooling kernel and the separate bias pass took a quarter of a step)."""
    from .. import _lib
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape[:-1] + (x.shape[-1] // 4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.disco_maxpool_last4(None, x.data_ptr(), bias.data_ptr(), x.numel() // x.shape[-1], x.shape[-1], x.shape[2], x.shape[1],
                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_maxpool_last4 failed ({rc})')
    return out


def _conv3x3_pool4_hip(x, w, b):
    """The stack's first block in one pass on the GPU (disco_conv3x3_pool4, csrc/k_crnn_conv.h): x (B, C_in, T, F) float32, folded
    weights w (C_out, C_in, 3, 3) and bias b (C_out,) -> (B, C_out, T - 2, F // 4), or None when the library has no direct form for the
    shape (the caller then runs the library convolution + disco_maxpool_last4)."""
    from .. import _lib
    lib = _lib.load()
    x = x.contiguous()
    B, Ci, T, F = x.shape
    out = torch.empty((B, w.shape[0], T - 2, F // 4), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.disco_conv3x3_pool4(None, x.data_ptr(), w.data_ptr(), b.data_ptr(), B, Ci, w.shape[0], T, F, out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    if rc == -2:                    # DISCO_E_UNSUPPORTED
        return None
    if rc != 0:
        raise RuntimeError(f'disco_conv3x3_pool4 failed ({rc})')
    return out


def crnn_features_hip(X, z, mic, pad, lo=STFT_MIN, hi=STFT_MAX, frames=None):
    """The networks' input features in one pass on the GPU (disco_crnn_features): X (R, K, T, F, M) complex64 spectra, z (R, K, T, F)
    complex64 compressed signals or None -> float32 (R K, C, pad[0] + T + pad[1], F), C = 1 (z None: |X[..., mic]|) or K (|X[..., mic]| then
    the |z| of the other nodes in node order, get_z_for_mask 'zs_hat'); clipped to [lo, hi], zero rows as padding (prepare_data pads after
    clipping).  What `predict_masks(..., prepared=True)` takes.
    frames: (R,) frames T_r <= T each ROOM has (Engine.frames; a host sequence, or an int32 tensor already on X's device), for a batch whose
    rooms differ in clip length (disco_crnn_features_rooms): the rows of the frames a room does not have are exact zeros like the padding
    -- not zeros clipped up to `lo` -- which is what the room's own padding holds when it is run alone."""
    from .. import _lib
    lib = _lib.load()
    R, K, T, F, M = X.shape
    assert X.is_contiguous() and X.dtype == torch.complex64 and (z is None or (z.is_contiguous() and tuple(z.shape) == (R, K, T, F)))
    C_ = 1 if z is None else K
    out = torch.empty((R * K, C_, pad[0] + T + pad[1], F), dtype=torch.float32, device=X.device)
    head = (None, X.data_ptr(), None if z is None else z.data_ptr(), R, K, M, T, F, int(mic), int(pad[0]), int(pad[1]), float(lo), float(hi))
    with torch.cuda.device(X.device):
        if frames is None:
            rc = lib.disco_crnn_features(*head, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        else:
            fr = _frames_on(frames, R, T, X.device, host=False)[1]
            rc = lib.disco_crnn_features_rooms(*head, fr.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_crnn_features{"" if frames is None else "_rooms"} failed ({rc})')
    return out


def _frames_on(frames, n, T, device, host=True):
    """`frames` (n values 0 <= T_b <= T: a host sequence, or an integer tensor) -> (int64 host array, int32 tensor on `device`).  host=False:
    a tensor that already lives on a GPU is taken as it is, unchecked, and no host copy is made of it (None comes back in its place).
    The device copy of a host sequence is made once per distinct content (_frames_dev): a batch that keeps its lengths from step to step
    issues no host-to-device copy after the first."""
    if torch.is_tensor(frames) and frames.is_cuda and not host:
        assert frames.numel() == n, (frames.numel(), n)
        return None, frames.to(device=device, dtype=torch.int32).contiguous().view(-1)
    h = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames).reshape(-1).astype(np.int64)
    if h.shape[0] != n or h.min() < 0 or h.max() > T:
        raise ValueError(f'frames: {n} values in [0, {T}] expected, got {h.shape[0]} in [{h.min()}, {h.max()}]')
    return h, _frames_dev(h.tobytes(), torch.device(device))


@functools.lru_cache(maxsize=16)
def _frames_dev(frames_bytes, device):
    return torch.from_numpy(np.frombuffer(frames_bytes, np.int64).astype(np.int32)).to(device)


@functools.lru_cache(maxsize=16)
def _compaction_plan(frames_bytes, T, chunk, device, by_index):
    """Layout of the existing frames of items of frames_bytes (int64 T_b) as compacted rows, item after item, made once per distinct content:
    row0 (B + 1,) host, rows of item b are [row0[b], row0[b + 1]); groups [(b0, b1)] of whole items of at most chunk * T rows (one item at
    the least); on `device`: row0 (B,) and the same counted from each group's first row (what the gather of a group takes), or, by_index,
    the (item, frame) of every row for the index gather."""
    fr = np.frombuffer(frames_bytes, np.int64)
    B = fr.shape[0]
    row0 = np.concatenate(([0], np.cumsum(fr)))
    groups, b0 = [], 0
    while b0 < B:
        b1 = b0 + 1
        while b1 < B and row0[b1 + 1] - row0[b0] <= chunk * T:
            b1 += 1
        groups.append((b0, b1))
        b0 = b1
    if by_index:
        tables = (np.repeat(np.arange(B), fr), np.concatenate([np.arange(n) for n in fr] + [np.zeros(0, np.int64)]))
    else:
        tables = (row0[:-1], np.concatenate([row0[a:b] - row0[a] for a, b in groups]))
    return row0, groups, tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.int64)).to(device) for t in tables)


def frames_to_pad(frame_to_pred=None, x_out=15):
    """(zero frames before, after) a sequence for `frame_to_pred` (get_frames_to_pad, speech_enhancement/utils.py:13-33)."""
    frame_to_pred = PRED_FRAME if frame_to_pred is None else frame_to_pred
    if frame_to_pred == 'mid':
        return (WIN_LEN // 2, WIN_LEN // 2)
    sel = (WIN_LEN + x_out) // 2
    return (sel - 1, WIN_LEN - sel)


def _crnn_windows_hip(feat, T, W, n_keep):
    """feat (nb, C, Tp, 4) contiguous float32 on the GPU -> (nb * T, n_keep): the leading n_keep floats of every window's
    flattened (C, W, 4) block (disco_crnn_windows)."""
    from .. import _lib
    lib = _lib.load()
    nb, C, Tp, Fy = feat.shape
    assert feat.is_contiguous() and Fy == 4
    out = torch.empty((nb * T, n_keep), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        rc = lib.disco_crnn_windows(None, feat.data_ptr(), nb, C, Tp, T, W, n_keep, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_crnn_windows failed ({rc})')
    return out


def _crnn_windows_rooms_hip(feat, T, W, n_keep, frames_sig, row0, n_rows):
    """feat (nb, C, Tp, 4) contiguous float32 on the GPU, frames_sig (nb,) int32 and row0 (nb,) int64 (its exclusive prefix sum) on the
    same device -> (n_rows, n_keep): the windows of the existing frames only, signal after signal (disco_crnn_windows_rooms)."""
    from .. import _lib
    lib = _lib.load()
    nb, C, Tp, Fy = feat.shape
    assert feat.is_contiguous() and Fy == 4 and frames_sig.dtype == torch.int32 and row0.dtype == torch.int64 and n_rows <= nb * T
    out = torch.empty((n_rows, n_keep), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        rc = lib.disco_crnn_windows_rooms(None, feat.data_ptr(), nb, C, Tp, T, W, n_keep, frames_sig.data_ptr(), row0.data_ptr(), out.data_ptr(),
                                          n_rows, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_crnn_windows_rooms failed ({rc})')
    return out


def _crnn_expand_rows_hip(rows, B, T, frames_sig, row0):
    """rows (n_rows, F) contiguous float32 on the GPU -> (B, T, F): row row0[b] + t at [b, t] for t < frames_sig[b], exact zeros in the
    frames a signal does not have (disco_crnn_expand_rows)."""
    from .. import _lib
    lib = _lib.load()
    n_rows, F = rows.shape
    assert rows.is_contiguous() and frames_sig.dtype == torch.int32 and row0.dtype == torch.int64
    out = torch.empty((B, T, F), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        rc = lib.disco_crnn_expand_rows(None, rows.data_ptr(), n_rows, B, T, F, frames_sig.data_ptr(), row0.data_ptr(), out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f'disco_crnn_expand_rows failed ({rc})')
    return out


# ---- training: the recurrent layer as GEMMs + the gate kernels, under autograd ---------------------------------------------------------------

def _stream_of(t):
    """The stream a kernel for tensor `t` goes to: the current one of t's device; 0 for a CPU tensor (a test driving the emulated library)."""
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


class _DeviceOf:
    """`with _DeviceOf(t):` -- torch.cuda.device(t.device) for a GPU tensor, nothing for a CPU tensor."""

    def __init__(self, t):
        self.ctx = torch.cuda.device(t.device) if t.is_cuda else None

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


def _use_kernels(t):
    """A GPU tensor always goes through the kernels (float32 only; a missing library is an error, not a fall-back).  A CPU tensor takes the
    same formulas in torch ops, unless a test has bound the emulated build by hand (_lib.takes_host_memory)."""
    from .. import _lib
    if t.is_cuda:
        if t.dtype != torch.float32:
            raise TypeError(f'the training kernels are float32, got {t.dtype}')
        return True
    return t.dtype == torch.float32 and _lib.takes_host_memory()


def _gru_step_train(g, gh, b_hh, h_prev, h_out, saved, kernels):
    """One forward step that keeps saved = [r | z | c | gh_n] (disco_gru_gates_train, or the same arithmetic in torch ops)."""
    n, H = h_out.shape
    if kernels:
        from .. import _lib
        assert g.stride(1) == 1 and (gh is None or gh.is_contiguous()) and h_out.is_contiguous() and saved.is_contiguous()
        with _DeviceOf(g):
            rc = _lib.load().disco_gru_gates_train(None, g.data_ptr(), g.stride(0), None if gh is None else gh.data_ptr(), b_hh.data_ptr(),
                                                   None if h_prev is None else h_prev.data_ptr(), h_out.data_ptr(), saved.data_ptr(), n, H,
                                                   _stream_of(g))
        if rc != 0:
            raise RuntimeError(f'disco_gru_gates_train failed ({rc})')
        return
    gh = b_hh.expand(n, -1) if gh is None else gh
    r = torch.sigmoid(g[:, :H] + gh[:, :H])
    z = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
    c = torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:])
    h_out.copy_((1 - z) * c if h_prev is None else (1 - z) * c + z * h_prev)
    saved.copy_(torch.cat((r, z, c, gh[:, 2 * H:]), 1))


def _gru_step_backward(d_out, d_carry, saved, h_prev, d_gi, d_gh, d_h, kernels):
    """One step of back-propagation through time (disco_gru_gates_backward, or the same arithmetic in torch ops): d_gi (a strided slice of
    the all-steps buffer), d_gh and d_h are written."""
    n, H = d_h.shape
    if kernels:
        from .. import _lib
        assert (d_out is None or d_out.stride(1) == 1) and (d_carry is None or d_carry.is_contiguous()) and d_gi.stride(1) == 1
        with _DeviceOf(saved):
            rc = _lib.load().disco_gru_gates_backward(None, None if d_out is None else d_out.data_ptr(), 0 if d_out is None else d_out.stride(0),
                                                      None if d_carry is None else d_carry.data_ptr(), saved.data_ptr(),
                                                      None if h_prev is None else h_prev.data_ptr(), d_gi.data_ptr(), d_gi.stride(0),
                                                      d_gh.data_ptr(), d_h.data_ptr(), n, H, _stream_of(saved))
        if rc != 0:
            raise RuntimeError(f'disco_gru_gates_backward failed ({rc})')
        return
    d = d_carry if d_out is None else (d_out if d_carry is None else d_out + d_carry)
    r, z, c, ghn = saved[:, :H], saved[:, H:2 * H], saved[:, 2 * H:3 * H], saved[:, 3 * H:]
    dn = d * (1 - z)
    dz = d * ((0 if h_prev is None else h_prev) - c)
    da_n = dn * (1 - c * c)
    da_z = dz * z * (1 - z)
    da_r = da_n * ghn * r * (1 - r)
    d_h.copy_(d * z)
    d_gi.copy_(torch.cat((da_r, da_z, da_n), 1))
    d_gh.copy_(torch.cat((da_r, da_z, da_n * r), 1))


class _GruTrain(torch.autograd.Function):
    """The one-layer GRU from a zero state over the leading `steps` steps of every sequence, as GEMMs plus the gate kernels; returns the
    hidden states of steps ff_out ... steps - 1 as (steps - ff_out, n, H) -- the loss frames, the only ones anything downstream reads.
    forward:  one GEMM for the input projections of all steps, then one recurrent GEMM + one disco_gru_gates_train per step.
    backward: one disco_gru_gates_backward per step in reverse order, with carry = d_h_direct + d_gh W_hh; the weight gradients are then
              single GEMMs over all steps at once: dW_hh = sum_t d_gh_t^T h_{t-1}, db_hh = sum_t d_gh_t, dW_ih, db_ih and dx from the
              (n steps, 3H) buffer of d_gi."""

    @staticmethod
    def forward(ctx, seq, w_ih, w_hh, b_ih, b_hh, ff_out):
        n, steps, n_in = seq.shape
        H = w_hh.shape[1]
        kernels = _use_kernels(seq)
        seq2 = seq.reshape(n * steps, n_in)
        gi = torch.addmm(b_ih, seq2, w_ih.t()).view(n, steps, 3 * H)
        hs = torch.empty((steps, n, H), dtype=seq.dtype, device=seq.device)
        saved = torch.empty((steps, n, 4 * H), dtype=seq.dtype, device=seq.device)
        b_hh = b_hh.contiguous()
        for t in range(steps):
            gh = None if t == 0 else torch.addmm(b_hh, hs[t - 1], w_hh.t())
            _gru_step_train(gi[:, t], gh, b_hh, None if t == 0 else hs[t - 1], hs[t], saved[t], kernels)
        ctx.save_for_backward(seq2, w_ih, w_hh, hs, saved)
        ctx.shape, ctx.ff_out, ctx.kernels = (n, steps, n_in), ff_out, kernels
        return hs[ff_out:].clone()

    @staticmethod
    def backward(ctx, d_hs):
        seq2, w_ih, w_hh, hs, saved = ctx.saved_tensors
        (n, steps, n_in), ff_out, kernels = ctx.shape, ctx.ff_out, ctx.kernels
        H = w_hh.shape[1]
        d_hs = d_hs.contiguous()
        d_gi = torch.empty((n, steps, 3 * H), dtype=hs.dtype, device=hs.device)
        d_gh = torch.empty((steps, n, 3 * H), dtype=hs.dtype, device=hs.device)
        carry = None
        for t in range(steps - 1, -1, -1):
            d_h = torch.empty((n, H), dtype=hs.dtype, device=hs.device)
            _gru_step_backward(d_hs[t - ff_out] if t >= ff_out else None, carry, saved[t], None if t == 0 else hs[t - 1], d_gi[:, t], d_gh[t], d_h,
                               kernels)
            if t > 0:
                carry = torch.addmm(d_h, d_gh[t], w_hh)
        d_gi2 = d_gi.view(n * steps, 3 * H)
        d_w_hh = d_gh[1:].reshape(-1, 3 * H).t() @ hs[:-1].reshape(-1, H) if steps > 1 else torch.zeros_like(w_hh)
        d_seq = (d_gi2 @ w_ih).view(n, steps, n_in) if ctx.needs_input_grad[0] else None
        return d_seq, d_gi2.t() @ seq2, d_w_hh, d_gi2.sum(0), d_gh.sum((0, 1)), None


class _Seq(nn.Module):
    """Holder that reproduces the reference's `<brick>.model = nn.Sequential(...)` key layout."""

    def __init__(self, *mods):
        super().__init__()
        self.model = nn.Sequential(*mods)

    def forward(self, x):
        return self.model(x)


class _RnnLayer(nn.Module):
    """`rnn.model.<i>.rnn_layer.*` (nn_structures.py RNNSingle): returns the sequence output only."""

    def __init__(self, input_size, hidden):
        super().__init__()
        self.rnn_layer = nn.GRU(input_size=input_size, hidden_size=hidden, num_layers=1, batch_first=True)

    def forward(self, x):
        return self.rnn_layer(x)[0]


class _FF(nn.Module):
    def __init__(self, n_in, n_out):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(n_in, n_out)])

    def forward(self, x):
        return torch.sigmoid(self.layers[0](x))


class CRNN(nn.Module):
    def __init__(self, n_ch=1, win_len=WIN_LEN, n_freq=257, cnn_filters=(32, 64, 64), rnn_units=256):
        super().__init__()
        self.input_shape = (n_ch, win_len, n_freq)
        chans = [n_ch, *cnn_filters]
        mods = []
        f = n_freq
        for i in range(len(cnn_filters)):
            mods += [nn.Conv2d(chans[i], chans[i + 1], kernel_size=3, stride=1, padding=(0, 1)),
                     nn.BatchNorm2d(chans[i + 1]), nn.MaxPool2d((1, 4))]
            f = f // 4
        self.cnn = _Seq(*mods)
        self.x_out = win_len - 2 * len(cnn_filters)                 # 15 frames survive the three unpadded 3x3 convolutions
        self.y_out = f                                              # 4 frequency cells after three (1,4) poolings
        self.rnn = _Seq(_RnnLayer(chans[-1] * self.y_out, rnn_units))
        self.ff = _FF(rnn_units, n_freq)
        self.fused_first_block = True       # predict_masks on the GPU: first conv block through disco_conv3x3_pool4 (False: library conv + pooling pass)

    # ---- the reference's evaluation (crnn.py:55-63)
    def forward(self, inp):
        if inp.dim() == 3:
            inp = inp.view(inp.size(0), 1, inp.size(1), inp.size(2))
        x = self.cnn(inp)
        x = x.view(x.size(0), x.size(2), x.size(1) * x.size(-1))    # NB: a re-interpretation, not a transpose (crnn.py:59)
        x = self.rnn(x)
        return self.ff(x.squeeze())

    def get_loss_frames(self, output_frames):
        """((first, last + 1) of the INPUT / label frames, (first, last + 1) of the OUTPUT frames) that the loss compares for
        'all' / 'mid' / 'last' (crnn.py:65-87): the convolutions drop 3 frames at either end of the 21."""
        from .utils import get_loss_frames
        win_len_in, win_len_out = self.input_shape[1], self.x_out
        if output_frames == 'last':
            ff_in = (win_len_in + win_len_out) // 2 - 1
            lf_in = ff_in + 1
        elif output_frames == 'mid':
            ff_in = int(np.ceil(win_len_in) / 2)
            lf_in = ff_in + 1
        elif output_frames == 'all':
            ff_in = (win_len_in - win_len_out) // 2
            lf_in = (win_len_in + win_len_out) // 2
        else:
            raise ValueError("Unknown argument value {}. It should be either 'all', 'mid' or 'last'.".format(output_frames))
        return (ff_in, lf_in), get_loss_frames(win_len_out, output_frames)

    # ---- the training route (dnn/train.py): the recurrent layer through the gate kernels, the output layer on the loss frames only
    def forward_train(self, x, output_frames='all'):
        """x (B, n_ch, 21, F) or (B, 21, F) -> (B, n_out, F): `forward(x)[:, ff_out:lf_out]` for the output frames of
        get_loss_frames(output_frames), differentiable, at a fraction of nn.GRU's cost on this shape.
        The convolution / BatchNorm / pooling modules are the same ones `forward` runs, under autograd: in train mode that is batch
        statistics, with the running statistics updated once per call exactly as `forward` updates them.  The reference's `.view`
        (crnn.py:59) follows.  The GRU is run as GEMMs plus the gate kernels (_GruTrain) over the steps up to the last loss frame only
        -- 8 for 'mid', 15 for 'all' and 'last' -- and the output layer and sigmoid on the loss frames only.
        There is no dropout to restate: the reference gives its RNN brick rnn_dropouts = 0.5 but builds the one-layer GRU with
        dropouts[-1] = 0 (nn_structures.py:124-126).
        CPU tensors take the same formulas in torch ops."""
        if x.dim() == 3:
            x = x.view(x.size(0), 1, x.size(1), x.size(2))
        f = self.cnn(x)
        f = f.view(f.size(0), f.size(2), f.size(1) * f.size(-1))    # NB: a re-interpretation, not a transpose (crnn.py:59)
        ff_out, lf_out = self.get_loss_frames(output_frames)[1]
        gru = self.rnn.model[0].rnn_layer
        hs = _GruTrain.apply(f[:, :lf_out], gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, ff_out)      # (n_out, B, H)
        return self.ff(hs).permute(1, 0, 2)

    def mid_frame(self):
        """Index of the output frame reshape_mask('mid') selects (tango.py:232-234)."""
        return int(np.floor(self.x_out / 2))

    @torch.no_grad()
    def predict_masks_windowed(self, mag, frame_to_pred=PRED_FRAME):
        """The reference's own evaluation order, kept for checking `predict_masks`: explicit 21-frame windows (prepare_data),
        the module's forward on every window, the selected output frame (reshape_mask).  mag (n_ch, T, F) -> (T, F)."""
        C, T, F = mag.shape
        W = self.x_out
        if frame_to_pred == 'mid':
            pad, sel = (WIN_LEN // 2, WIN_LEN // 2), int(np.floor(W / 2))
        else:
            s_ = (WIN_LEN + W) // 2
            pad, sel = (s_ - 1, WIN_LEN - s_), W - 1
        x = torch.nn.functional.pad(torch.clamp(mag, STFT_MIN, STFT_MAX), (0, 0, pad[0], pad[1]))
        wins = x.unfold(1, WIN_LEN, 1).permute(1, 0, 3, 2)          # (T, C, 21, F)
        return self.forward(wins.contiguous())[:, sel, :]

    def _cnn_folded(self, x, compute_dtype=None):
        """compute_dtype (torch.bfloat16 / torch.float16): the convolutions run in that type (inputs, weights and feature maps;
        MIOpen accumulates in float32), the result is returned in float32.  None: float32 throughout.
        The convolutional stack with every BatchNorm2d (inference statistics) folded into the convolution before it:
        w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta -- the same function, one kernel less per
        layer (MIOpen's inference batch-norm was 10 % of the GPU time of a step).  Folded weights are cached per parameter
        version, so loading a checkpoint afterwards is picked up."""
        mods = list(self.cnn.model)
        key = tuple((p.data_ptr(), p._version) for m in mods for p in list(m.parameters()) + list(m.buffers()))
        if getattr(self, '_fold_key', None) != key:
            folded = []
            for conv, bn in zip(mods[0::3], mods[1::3]):
                g = bn.weight / torch.sqrt(bn.running_var + bn.eps)
                folded.append(((conv.weight * g.view(-1, 1, 1, 1)).contiguous(), ((conv.bias - bn.running_mean) * g + bn.bias).contiguous(),
                               conv.padding))
            self._folded, self._fold_key = folded, key
            self._folded_lp = {}
        if compute_dtype is not None and x.dtype != compute_dtype:
            lp = self._folded_lp.get(compute_dtype)
            if lp is None:
                lp = self._folded_lp[compute_dtype] = [(w.to(compute_dtype), b.to(compute_dtype), pad) for w, b, pad in self._folded]
            x = x.to(compute_dtype)
            for (w, b, pad), pool in zip(lp, mods[2::3]):
                x = pool(torch.nn.functional.conv2d(x, w, b, stride=1, padding=pad))
            return x.float()
        for i, ((w, b, pad), pool) in enumerate(zip(self._folded, mods[2::3])):
            if x.is_cuda and x.dtype == torch.float32 and tuple(pool.kernel_size) == (1, 4):
                if i == 0 and self.fused_first_block and tuple(pad) == (0, 1) and tuple(w.shape[2:]) == (3, 3):
                    # few input channels, 257 bins: bound by its un-pooled output, which the fused kernel never writes (csrc/k_crnn_conv.h)
                    y = _conv3x3_pool4_hip(x, w, b)
                    if y is not None:
                        x = y
                        continue
                x = _maxpool4_hip(torch.nn.functional.conv2d(x, w, None, stride=1, padding=pad), b)      # bias added after the max
            else:
                x = pool(torch.nn.functional.conv2d(x, w, b, stride=1, padding=pad))
        return x

    # ---- sequence evaluation
    @torch.no_grad()
    def predict_masks(self, mag, chunk=256, frame_to_pred=PRED_FRAME, norm_type=None, compute_dtype=None, prepared=False, frames=None):
        """mag: (B, n_ch, T, F) magnitudes (un-clipped |STFT| of the node's reference mic, then |z| of the other nodes)
        -> masks (B, T, F), equal to reshape_mask(model(prepare_data(..., frame_to_pred, norm_type)), frame_to_pred) of the
        reference for every item (speech_enhancement/utils.py:13-66, 69-138; tango.py:228-240).
        frame_to_pred: 'mid' (tango.py:35, what offline_tango uses) or 'last' (prepare_data's own default);
        norm_type: None | 'scale_to_unit_norm' | 'scale_to_1' | 'center_and_scale' (per frequency over the whole sequence,
        utils.py:36-66; 'pcen' is librosa's and not offered).
        compute_dtype: None (float32, the default and what the parity tests pin) or torch.bfloat16 / torch.float16 -- the
        convolutions and the GRU / output GEMMs take their inputs in that type and accumulate in float32 (matrix cores at full
        rate instead of the float32 rate); the gate arithmetic, the recurrent state and the masks stay float32.  An explicit
        accuracy-for-speed switch: bench.py's C4_bf16 entry states the mask error it costs against the float32 evaluation.
        prepared=True: `mag` is ALREADY clipped and zero-padded for `frame_to_pred` (crnn_features_hip: (B, n_ch, pad + T + pad, F)); norm_type None only.
        frames: None, or B frame counts T_b <= T (a host sequence; a tensor on a GPU is copied to the host) for items of different lengths
        in one rectangular batch: item b comes out as `predict_masks(mag[b:b + 1, :, :T_b])` does, with exact zeros at t >= T_b.  The rows
        t >= T_b are zeroed after the clamp (prepared=True: the caller did, crnn_features_hip(..., frames=...)), so that the convolutions, which
        have no padding along time, see what the item's own zero padding would hold; the window gather, the GRU steps and the output layer
        then run on the sum(T_b) existing frames only.  norm_type must be None with frames: no caller needs the per-frequency statistics
        over a ragged batch, and they would have to be taken over every item's own frames."""
        if self.training:
            raise RuntimeError('predict_masks is the inference path (BatchNorm folded on its running statistics): call model.eval() first')
        B, C, T, F = mag.shape
        if prepared:
            if norm_type is not None:
                raise ValueError('prepared features are clipped and padded only: norm_type must be None')
            T -= sum(frames_to_pad(frame_to_pred, self.x_out))
        W = self.x_out                                              # 15 output frames per 21-frame window
        if frame_to_pred == 'mid':                                  # get_frames_to_pad (utils.py:13-33), reshape_mask (tango.py:228-240)
            pad = (WIN_LEN // 2, WIN_LEN // 2)
            steps = int(np.floor(W / 2)) + 1                        # GRU steps needed to reach the selected output frame
        elif frame_to_pred == 'last':
            sel = (WIN_LEN + W) // 2
            pad = (sel - 1, WIN_LEN - sel)
            steps = W
        else:
            raise ValueError(":param output_frames: should be 'mid' or 'last' ('all' is not implemented in the reference either)")
        if frames is not None:
            if norm_type is not None:
                raise ValueError('frames (items of different lengths) with a norm_type: the statistics over a ragged batch are not offered')
            fr, fr_dev = _frames_on(frames, B, T, mag.device)
        x = mag if prepared else torch.clamp(mag, STFT_MIN, STFT_MAX)      # normalization(): clip first, whatever the type
        if frames is not None and not prepared:                          # the frames an item does not have: zeros, as its own padding would be
            x = x.masked_fill((torch.arange(T, device=mag.device) >= fr_dev.view(B, 1))[:, None, :, None], 0.0)
        if norm_type == 'scale_to_unit_norm':
            x = x / torch.linalg.vector_norm(x, dim=2, keepdim=True)
        elif norm_type == 'scale_to_1':
            x = x / torch.quantile(x, 0.99, dim=2, keepdim=True)
        elif norm_type == 'center_and_scale':
            x = x - x.mean(dim=2, keepdim=True)
            x = x / x.std(dim=2, keepdim=True, unbiased=False)
        elif norm_type is not None:
            raise NotImplementedError(f"norm_type '{norm_type}' (librosa's pcen is third-party and absent)")
        if not prepared:
            x = torch.nn.functional.pad(x, (0, 0, pad[0], pad[1]))  # zeros AFTER clipping / scaling, as prepare_data does
        feat = self._cnn_folded(x, compute_dtype)                   # (B, 64, T + 20 - 6, 4)
        Cc, Fy = feat.shape[1], self.y_out
        # The reference's `.view` (crnn.py:59) re-interprets each window's (64, 15, 4) block as (15, 256) WITHOUT a transpose:
        # GRU step s reads elements [256 s, 256 (s + 1)) of the flattened block, i.e. only the first ceil(256 steps / 60)
        # channels matter for the `steps` steps that are run.
        c_used = min(Cc, -(-(steps * Cc * Fy) // (W * Fy)))
        gru = self.rnn.model[0].rnn_layer
        H = gru.hidden_size
        w_ih, w_hh, b_ih, b_hh = gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0
        if compute_dtype is not None:
            w_ih_t, w_hh_t = w_ih.t().to(compute_dtype), w_hh.t().to(compute_dtype)

            def gemm(bias, a, wt):                                  # float32 out = bias + a @ wt with low-precision operands
                a = a.to(compute_dtype)
                try:
                    return torch.addmm(bias, a, wt, out_dtype=torch.float32)
                except (TypeError, RuntimeError):
                    return torch.addmm(bias.to(compute_dtype), a, wt).float()
        else:
            w_ih_t, w_hh_t = w_ih.t(), w_hh.t()

            def gemm(bias, a, wt):
                return torch.addmm(bias, a, wt)
        feat = feat.contiguous()
        sB, sC = feat.stride(0), feat.stride(1)
        n_keep = steps * Cc * Fy
        hip = feat.is_cuda and feat.dtype == torch.float32 and Fy == 4

        def gru_ff(seq):
            """seq (n, steps, Cc Fy): the windows' leading GRU inputs -> (n, F) masks of the selected output frame"""
            # The GRU over `steps` steps from a zero state, for all n windows at once, as plain GEMMs: one for the input
            # projections of every step, one per step for the recurrent part (torch's / MIOpen's nn.GRU kernel is an order of
            # magnitude slower on this shape: a quarter of a million 8-step sequences).  Gate order r, z, n; same arithmetic.
            n = seq.shape[0]
            gi = gemm(b_ih, seq.reshape(-1, Cc * Fy), w_ih_t).view(n, steps, 3 * H)
            fused = gi.is_cuda and gi.dtype == torch.float32          # pointwise gate math in one HIP kernel (libdisco_hip.so)
            h = None
            for st in range(steps):
                g = gi[:, st]
                if fused:
                    gh = None if h is None else gemm(b_hh, h, w_hh_t)
                    h = _gru_gates_hip(g, gh, b_hh, h, H)
                    continue
                gh = b_hh.expand(n, -1) if h is None else gemm(b_hh, h, w_hh_t)
                r = torch.sigmoid(g[:, :H] + gh[:, :H])
                zg = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
                nn_ = torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:])
                h = (1 - zg) * nn_ if h is None else torch.addcmul((1 - zg) * nn_, zg, h)
            return self.ff(h)

        if frames is not None:
            return self._masks_of_existing_frames(feat, fr, fr_dev, T, F, chunk, c_used, n_keep, hip, gru_ff, mag.dtype)
        out = torch.empty((B, T, F), dtype=mag.dtype, device=mag.device)
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            # window i of channel c = frames i .. i+14 of that channel = W * Fy CONTIGUOUS floats starting at i * Fy: an
            # overlapping strided view, gathered into rows (c, w, fy) with 60-float runs (a permuted unfold of the same
            # data copies element by element and was the slowest kernel of the whole step)
            if hip:
                seq = _crnn_windows_hip(feat[b0:b0 + nb], T, W, n_keep).view(nb * T, steps, Cc * Fy)
            else:
                win = feat[b0:b0 + nb].as_strided((nb, T, c_used, W * Fy), (sB, Fy, sC, 1)).reshape(nb * T, c_used * W * Fy)
                seq = win[:, :n_keep].view(nb * T, steps, Cc * Fy)
            out[b0:b0 + chunk] = gru_ff(seq).view(nb, T, F)
        return out

    def _masks_of_existing_frames(self, feat, fr, fr_dev, T, F, chunk, c_used, n_keep, hip, gru_ff, dtype):
        """predict_masks' second half for items of different lengths: the recurrent layer and the output layer on the sum(fr) existing frames,
        compacted item after item (row0 = exclusive prefix sum of fr), in groups of whole items of at most chunk * T rows -- the input
        projections of a group are as large as those of `chunk` full items -- and the rows put back at [b, t] with zeros beyond fr[b]."""
        B, Cc, _, Fy = feat.shape
        W, dev = self.x_out, feat.device
        steps = n_keep // (Cc * Fy)
        row0, groups, tables = _compaction_plan(fr.tobytes(), T, chunk, dev, not hip)
        N = int(row0[-1])
        if N == 0:
            return torch.zeros((B, T, F), dtype=dtype, device=dev)
        rows = torch.empty((N, F), dtype=torch.float32 if hip else dtype, device=dev)
        if hip:
            row0_dev, rel_dev = tables                              # rel: every group's rows count from its own buffer's start
        else:
            b_idx, t_idx = tables
            win = feat.as_strided((B, T, c_used, W * Fy), (feat.stride(0), Fy, feat.stride(1), 1))
        for a, b in groups:
            r0, r1 = int(row0[a]), int(row0[b])
            if r1 == r0:
                continue
            if hip:
                seq = _crnn_windows_rooms_hip(feat[a:b], T, W, n_keep, fr_dev[a:b], rel_dev[a:b], r1 - r0)
            else:                                                   # the same rows by index: window t of item b, its leading n_keep floats
                seq = win[b_idx[r0:r1], t_idx[r0:r1]].reshape(r1 - r0, c_used * W * Fy)[:, :n_keep]
            rows[r0:r1] = gru_ff(seq.reshape(r1 - r0, steps, Cc * Fy))
        if hip:
            return _crnn_expand_rows_hip(rows, B, T, fr_dev, row0_dev).to(dtype)
        out = torch.zeros((B, T, F), dtype=dtype, device=dev)
        out[b_idx, t_idx] = rows
        return out


def flops_per_frame(n_ch=1, n_freq=257, cnn_filters=(32, 64, 64), rnn_units=256, frame_to_pred=PRED_FRAME):
    """Multiply-add FLOPs (2 per MAC) `predict_masks` spends per output frame of one signal: the three 3x3 convolutions evaluated
    once over the sequence (not once per 21-frame window), the GRU steps that reach the selected output frame (8 for 'mid', 15 for
    'last') as an input-projection GEMM + one recurrent GEMM per step after the first, and the output layer."""
    chans = [n_ch, *cnn_filters]
    macs, f = 0, n_freq
    for i in range(len(cnn_filters)):
        macs += f * chans[i + 1] * chans[i] * 9
        f //= 4
    steps = (WIN_LEN - 2 * len(cnn_filters)) // 2 + 1 if frame_to_pred == 'mid' else WIN_LEN - 2 * len(cnn_filters)
    n_in = chans[-1] * f
    macs += steps * n_in * 3 * rnn_units + (steps - 1) * rnn_units * 3 * rnn_units + rnn_units * n_freq
    return 2 * macs


def build_crnn(n_ch=1, device=None, state_dict=None):
    """CRNN with the constructor arguments of tango.py:124-129; optionally loads a reference checkpoint's
    `model_state_dict` (train.py:151-156)."""
    model = CRNN(n_ch=n_ch)
    if state_dict is not None:
        model.load_state_dict(state_dict)
    if device is not None:
        model = model.to(device)
    return model.eval()


def get_z_for_mask(z_s, z_n, k, nb_nodes, z_sigs='zs_hat'):
    """tango.py:158-186 -- which compressed signals feed the step-2 network of node k.  z_s, z_n: (K, ...) arrays/tensors."""
    if z_sigs in ('zs_hat', 'zn_hat'):
        z_in = z_s if z_sigs == 'zs_hat' else z_n
        idx = [j for j in range(nb_nodes) if j != k]
        return z_in[idx]
    cat = torch.cat if torch.is_tensor(z_s) else np.concatenate
    z_in = cat((z_s, z_n), 0)
    n = z_in.shape[0]
    order = [i // 2 if i % 2 == 0 else int(0.5 * (n - 1 + i)) for i in range(n)]      # interleave zs_j, zn_j as in training
    z_out = z_in[order]
    keep = [i for i in range(2 * nb_nodes) if i not in (2 * k, 2 * k + 1)]
    return z_out[keep]
