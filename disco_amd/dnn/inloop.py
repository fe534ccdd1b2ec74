"""The two-step MWF with DNN-predicted masks in the loop (BASELINE.json configs[3]; tango.py:209-215, 387-394):
mask_z = CRNN(|Y_ref|) before step 1, mask_w = CRNN([|Y_ref| ; |z_j|, j != k]) between the steps.  Everything stays on
the GPU: the STFT / covariance / solve / filter / iSTFT are the HIP kernels (through the C ABI, zero-copy on torch
tensors), the CRNN is PyTorch-ROCm."""
import numpy as np
import torch

from .crnn import crnn_features_hip, frames_to_pad


def _c64(t):
    """float32 (..., 2) view <-> complex64 helpers stay zero-copy."""
    return torch.view_as_complex(t)


def tango_enhance_dnn(eng, y, model_z, model_w=None, want_masks=False, dnn_chunk=512, mark=None, compute_dtype=None, masks=None, want_yf=False):
    """eng: disco_amd.engine.Engine (rooms R, nodes K, mics M); y: torch float32 (R, K, M, L) on the engine's device.
    model_z: CRNN(n_ch=1); model_w: CRNN(n_ch=K) or None (= reuse mask_z, tango.py:388-389).
    compute_dtype: None (float32) or torch.bfloat16 / torch.float16 for the networks' convolutions and GEMMs (CRNN.predict_masks).
    dnn_chunk: signals per GRU pass (the input projections of a pass are 8 x 768 floats per frame: 15 MB per ten-second signal); 500 signals in one
    pass measured 74.0 ms per C4 step against 76.7 at 64 (larger rocBLAS products).
    mark: optional callable(name) invoked after every phase (stft, crnn_z, cov1, solve1, apply1, crnn_w, step2_cov, solve2,
    step2_apply_istft) -- bench.py records an event on the launch stream in it to time the phases.
    masks: optional (mask_z, mask_w) float32 (R, K, T, F) tensors used INSTEAD of the networks' predictions (the same kernel sequence on
    given masks: how bench.py re-derives the spectra of a timed step).  want_yf: the filtered spectra (R, K, T, F) complex64 come back
    as the last element; the final filter and the iSTFT then run as two calls (the one-pass kernel keeps yf on chip).
    Per-room clip lengths (eng.set_lengths): both networks see every room as if it were alone at its own length -- the features of the frames
    t >= T_r a room does not have are exact zeros (crnn_features_hip(..., frames=...)), the recurrent and output layers run on the existing
    frames only (predict_masks(..., frames=...)) -- the returned masks are zero at t >= T_r and `out` is zero at and beyond L_r.
    Returns out (R, K, L) torch float32 [, mask_z, mask_w (R, K, T, F)][, yf]."""
    mark = mark or (lambda name: None)
    lib, ctx = eng.lib, eng.ctx
    R, K, M, L, T, F = eng.R, eng.K, eng.M, eng.Lsamp, eng.T, eng.F
    dev = y.device
    G = R * K
    p = lambda t: t.data_ptr()
    X = torch.empty((R, K, T, F, M, 2), dtype=torch.float32, device=dev)
    eng._chk(lib.disco_stft(ctx, p(y), G, M, p(X), None))
    mark('stft')
    Xc = _c64(X)                                                       # (R, K, T, F, M) complex64 view
    ref = eng.cfg.ref_mic
    # rooms of different clip lengths: T_r per room for the features, per signal (room, node) for the networks; None = the uniform batch
    fr_room = None if eng._lengths is None else eng.frames
    fr_sig = {} if fr_room is None else {'frames': np.repeat(fr_room, K)}
    if masks is not None:
        mask_z = masks[0].contiguous()
    else:
        # |Y| at the reference mic (tango.py:338), clipped and padded for the window selection (prepare_data) in one pass
        feat = crnn_features_hip(Xc, None, ref, frames_to_pad(None, model_z.x_out), frames=fr_room)
        mask_z = model_z.predict_masks(feat, chunk=dnn_chunk, compute_dtype=compute_dtype, prepared=True, **fr_sig).reshape(R, K, T, F).contiguous()
        del feat
    mark('crnn_z')
    eng._chk(lib.disco_cov_masked(ctx, p(X), p(mask_z), None, None, 0, M, None, None, None))
    mark('cov1')
    w_loc = torch.empty((R, K, F, M, 2), dtype=torch.float32, device=dev)
    eng._chk(lib.disco_gevd_mwf_r1_pending(ctx, eng.cfg.mu, p(w_loc), None, None))
    mark('solve1')
    if masks is not None and K > 1:
        mask_w = masks[1].contiguous()
    elif model_w is None or K == 1:
        mask_w = mask_z
    else:
        z = torch.empty((R, K, T, F, 2), dtype=torch.float32, device=dev)
        eng._chk(lib.disco_apply(ctx, p(X), None, p(w_loc), M, 1, p(z), None))
        mark('apply1')
        # step 2 always looks at channel 0 (tango.py:391), then the |z| of the other nodes in node order (get_z_for_mask 'zs_hat', :158-186)
        feat = crnn_features_hip(Xc, _c64(z), 0, frames_to_pad(None, model_w.x_out), frames=fr_room)
        mask_w = model_w.predict_masks(feat, chunk=dnn_chunk, compute_dtype=compute_dtype, prepared=True, **fr_sig).reshape(R, K, T, F).contiguous()
        del feat
        mark('crnn_w')
    out = torch.empty((R, K, L), dtype=torch.float32, device=dev)
    yf = None
    if K == 1:
        # single node: step 2 repeats step 1 on the same statistics (tango.py K = 1) -> iSTFT of z
        z = torch.empty((R, K, T, F, 2), dtype=torch.float32, device=dev)
        eng._chk(lib.disco_apply(ctx, p(X), None, p(w_loc), M, 1, p(z), None))
        eng._chk(lib.disco_istft(ctx, p(z), G, p(out), None))
        yf = z
        mark('apply_istft')
    else:
        eng._chk(lib.disco_step2_cov_fused(ctx, p(X), p(mask_w), p(w_loc), None, None, None, None))
        mark('step2_cov')
        w_glo = torch.empty((R, K, F, M + K - 1, 2), dtype=torch.float32, device=dev)
        eng._chk(lib.disco_gevd_mwf_r1_pending(ctx, eng.cfg.mu, p(w_glo), None, None))
        mark('solve2')
        rc = -2 if want_yf else lib.disco_step2_apply_istft_fused(ctx, p(X), p(w_loc), p(w_glo), p(out), None)
        if rc != 0:                                                    # shapes outside the fused kernel: two calls
            yf = torch.empty((R, K, T, F, 2), dtype=torch.float32, device=dev)
            eng._chk(lib.disco_step2_apply_fused(ctx, p(X), p(w_loc), p(w_glo), None, p(yf), None))
            eng._chk(lib.disco_istft(ctx, p(yf), G, p(out), None))
        mark('step2_apply_istft')
    res = (out, mask_z, mask_w) if want_masks else (out,)
    if want_yf:
        res = res + (_c64(yf),)
    return res if len(res) > 1 else out
