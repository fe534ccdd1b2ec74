"""The training loss of the mask estimators (disco_theque/dnn/engine/losses.py): `nanmean` and `reconstruction_loss` with the reference's
surface, in plain torch, and `recon_loss_frames`, the same loss on the frames `get_x_for_loss` selects, computed by two HIP kernels
(disco_recon_loss / disco_recon_loss_grad) without slicing the three tensors."""
import torch

from .crnn import _DeviceOf, _stream_of, _use_kernels


def nanmean(v, *args, inplace=False, **kwargs):
    """Mean over the non-NaN entries (losses.py:4-12)."""
    if not inplace:
        v = v.clone()
    is_nan = torch.isnan(v)
    v[is_nan] = 0
    return v.sum(*args, **kwargs) / (~is_nan).float().sum(*args, **kwargs)


def reconstruction_loss(y_true, y_pred, y_in):
    """MSE of the mask applied to the input magnitudes (losses.py:15-25): nanmean(((y_pred - y_true) y_in)^2)."""
    return nanmean(((y_pred - y_true) * y_in) ** 2)


class _ReconLossFrames(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, y, x, ff_in):
        from .. import _lib
        lib = _lib.load()
        est, y, x = est.contiguous(), y.contiguous(), x.contiguous()
        B, n_out, F = est.shape
        C, W = x.shape[1], x.shape[2]
        assert est.dtype == y.dtype == x.dtype == torch.float32 and tuple(y.shape) == (B, W, F) and tuple(x.shape) == (B, C, W, F)
        sums = torch.empty(2, dtype=torch.float64, device=est.device)
        ws = torch.empty(_lib.RECON_LOSS_WS_BYTES // 8, dtype=torch.float64, device=est.device)
        with _DeviceOf(est):
            rc = lib.disco_recon_loss(None, est.data_ptr(), y.data_ptr(), x.data_ptr(), B, C, W, F, int(ff_in), n_out, sums.data_ptr(), ws.data_ptr(),
                                      _lib.RECON_LOSS_WS_BYTES, _stream_of(est))
        if rc != 0:
            raise RuntimeError(f'disco_recon_loss failed ({rc})')
        ctx.save_for_backward(est, y, x, sums)
        ctx.ff_in = int(ff_in)
        return (sums[0] / sums[1]).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        from .. import _lib
        lib = _lib.load()
        est, y, x, sums = ctx.saved_tensors
        B, n_out, F = est.shape
        g = g.to(torch.float32).contiguous()
        d_est = torch.empty_like(est)
        with _DeviceOf(est):
            rc = lib.disco_recon_loss_grad(None, est.data_ptr(), y.data_ptr(), x.data_ptr(), B, x.shape[1], x.shape[2], F, ctx.ff_in, n_out,
                                           sums.data_ptr(), g.data_ptr(), d_est.data_ptr(), _stream_of(est))
        if rc != 0:
            raise RuntimeError(f'disco_recon_loss_grad failed ({rc})')
        return d_est, None, None, None


def recon_loss_frames(est, y, x, ff_in):
    """reconstruction_loss on the loss frames: est (B, n_out, F) the network's output on those frames, label y (B, W, F), input x (B, C, W, F)
    or (B, W, F) whose channel 0 weights the loss (dnn/utils.py:237); term (b, j, f) = ((est[b, j, f] - y[b, ff_in + j, f]) x[b, 0, ff_in + j, f])^2.
    float32 scalar, differentiable in `est` only (labels and inputs are data).  Every term is formed and summed in float64 in a fixed order:
    two calls give the same bits.
    One stated difference from the reference: the gradient is an exact 0 where a term is NaN.  The reference's autograd multiplies the zeroed
    entry's 0 gradient by the NaN operand and leaves NaN there; such terms only arise once the network has already diverged.
    CPU tensors: the plain torch expression in the tensors' own type, as the reference."""
    if x.dim() == 3:
        x = x.unsqueeze(1)
    n_out = est.shape[1]
    if not _use_kernels(est):
        return reconstruction_loss(y[:, ff_in:ff_in + n_out], est, x[:, 0, ff_in:ff_in + n_out])
    return _ReconLossFrames.apply(est, y, x, ff_in)
