"""Python driver of the HIP engine: one `Engine` = one `disco_ctx` (one device, one batch geometry).

Arrays may be given as numpy arrays (copied host->device through the library's own hipMemcpy), as `DevBuf`
(device resident, returned by every method), or as torch ROCm tensors (zero-copy through `data_ptr()`).
All compute happens in libdisco_hip.so; this file only marshals pointers.  No CPU fallback exists.
The marshalling is stated once, in the helpers under "plumbing": `_out` (caller-owned or fresh output), `_alias` (a second argument that
may be the first), `_ptr` (optional buffer -> pointer or NULL), `_span_stops` / `_span_stops_dev` (`stop` of a metric), `_chunk_plan` /
`_chunks` (a batch walked under a workspace budget), `_pencils` (the solvers' prologue), `_selftest_pair`, `_on_host` / `_lead_stops` / `_lead_values`
(the container rule, the `stop` and the other per-signal values over leading axes of vad_samples / mix_scaled / noise_from_signal /
affine_segment); each method names its dialect.
"""
import ctypes as C

import numpy as np

from . import _lib as L


class DiscoError(RuntimeError):
    pass


class DevBuf:
    """A device allocation owned by an Engine, with shape/dtype metadata."""

    def __init__(self, eng, shape, dtype):
        self.eng = eng
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        eng._chk(eng.lib.disco_dev_alloc(eng.ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        self.eng._chk(self.eng.lib.disco_d2h(self.eng.ctx, out.ctypes.data, self.ptr, self.nbytes, None))
        self.eng.sync()
        return out

    def reshape(self, *shape):
        v = object.__new__(DevBuf)
        v.eng, v.dtype, v.nbytes, v.ptr = self.eng, self.dtype, self.nbytes, self.ptr
        v.shape = tuple(int(s) for s in shape)
        if v.shape.count(-1) == 1:                       # one free axis, as numpy's reshape
            known = -int(np.prod(v.shape, dtype=np.int64))
            v.shape = tuple(self.nbytes // self.dtype.itemsize // max(known, 1) if s == -1 else s for s in v.shape)
        v._base = self
        assert int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize == self.nbytes
        return v

    def part(self, start, shape):
        """A view of prod(shape) elements that begins at flat element `start`: the memory stays owned by this buffer."""
        v = object.__new__(DevBuf)
        v.eng, v.dtype, v.shape = self.eng, self.dtype, tuple(int(s) for s in shape)
        v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize
        assert 0 <= start and int(start) * v.dtype.itemsize + v.nbytes <= self.nbytes, (start, shape, self.shape)
        v.ptr = self.ptr + int(start) * v.dtype.itemsize
        v._base = self
        return v

    def __getitem__(self, i):
        """buf[i], i an integer: the contiguous block at index i of the leading axis, as a view."""
        n = self.shape[0]
        i = int(i) + (n if int(i) < 0 else 0)
        if not 0 <= i < n:
            raise IndexError(f'index {i} out of range for a leading axis of {n}')
        return self.part(i * int(np.prod(self.shape[1:], dtype=np.int64)), self.shape[1:])

    def free(self):
        if getattr(self, 'ptr', None) and not hasattr(self, '_base'):
            self.eng.lib.disco_dev_free(self.eng.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.eng.ctx:
                self.free()
        except Exception:
            pass


def _ptr(buf):
    """Device pointer of an optional output the method allocated, NULL for one not asked for."""
    return buf.ptr if buf is not None else None


def _on_host(a):
    """Neither a DevBuf nor a torch tensor: a NumPy array or whatever np.asarray takes -- a method that follows the container rule
    (NumPy in, NumPy out; device in, DevBuf out) answers such an input with a NumPy array."""
    return not (isinstance(a, DevBuf) or hasattr(a, 'data_ptr'))


def parse_mask_type(mask):
    """'irm1' -> (DISCO_MASK_IRM, 1); raises ValueError like tango.py:223 / dnn/utils.py:69."""
    if not isinstance(mask, str) or len(mask) != 4 or mask[:3] not in L.MASK_TYPES or not mask[3].isdigit():
        raise ValueError('Unknown mask type. Should be "irmX", "ibmX" or "iamX"')
    return L.MASK_TYPES[mask[:3]], int(mask[3])


STOI_FS = 10000


def stoi_resample_taps(fs_sig):
    """-> (p, q, h): 10000 / fs_sig in lowest terms and the anti-aliasing filter pystoi's resample_oct hands to scipy.signal.resample_poly
    as `window` (Kaiser-windowed sinc, 60 dB rejection, cut-off 1 / (2 max(p, q)), normalised to unit sum); 2 L + 1 float64 taps
    (581 at 16 kHz).  At 10 kHz: (1, 1, one tap), nothing is resampled."""
    if int(fs_sig) != fs_sig or fs_sig < 1:
        raise ValueError(f'fs_sig must be a positive integer number of Hz: {fs_sig}')
    g = int(np.gcd(STOI_FS, int(fs_sig)))
    p, q = STOI_FS // g, int(fs_sig) // g
    if p == q:
        return 1, 1, np.ones(1)
    fc = 1.0 / (2 * max(p, q))
    half = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2 * p * fc * np.sinc(2 * fc * t))
    return p, q, h / np.sum(h)


class Engine:
    def __init__(self, rooms, nodes, mics, length, n_fft=512, hop=None, ref_mic=0, mask='irm1', bin_thr=0.0,
                 mu=1.0, pad_mode='reflect', device=0, lib=None, staged_step2=False, lazy_scratch=False):
        self.lib = lib if lib is not None else L.load()
        mt, mp = parse_mask_type(mask)
        hop = n_fft // 2 if hop is None else hop
        self.cfg = L.DiscoCfg(rooms=rooms, nodes=nodes, mics=mics, length=length, n_fft=n_fft, hop=hop,
                              ref_mic=ref_mic, mask_type=mt, mask_pow=mp, mask_bin_thr_db=bin_thr, mu=mu,
                              pad_mode=L.PAD_MODES[pad_mode], device=device,
                              flags=(L.FLAG_STAGED_STEP2 if staged_step2 else 0) | (L.FLAG_LAZY_SCRATCH if lazy_scratch else 0))
        ctx = C.c_void_p()
        rc = self.lib.disco_create(C.byref(ctx), C.byref(self.cfg))
        self.ctx = ctx.value if rc == 0 else None
        if rc != 0:
            raise DiscoError(f'disco_create failed ({rc}): {self.lib.disco_last_error(None).decode()}')
        self.R, self.K, self.M, self.Lsamp = rooms, nodes, mics, length
        self.n_fft, self.device, self.pad_mode = n_fft, device, pad_mode
        self.Kl, self.k0 = nodes, 0                     # node shard held by this engine (all nodes by default)
        self.zblk = nodes                               # layout of exchanged-signal arguments (set_z_blocks)
        self.T = self.lib.disco_n_frames(self.ctx)
        self.F = self.lib.disco_n_freq(self.ctx)
        self.stream = None
        self._tuning = (0, 0, 0, 0)                     # what set_tuning pinned (the library has no getter)
        self._lengths = None                            # per-room clip lengths (set_lengths; None = the uniform batch)
        self._ctor = dict(mics=mics, length=length, n_fft=n_fft, hop=hop, ref_mic=ref_mic, mask=mask, bin_thr=bin_thr, mu=mu,
                          pad_mode=pad_mode, device=device, staged_step2=staged_step2, lazy_scratch=lazy_scratch)
        # the hipemu TEST build (tests/emu_build.py) keeps "device" memory on the host: CPU torch tensors are legitimate there
        self._host_pointers_ok = b'gfx950' not in self.lib.disco_version()

    # ---- plumbing
    def _chk(self, rc):
        if rc != 0:
            raise DiscoError(f'libdisco_hip error {rc}: {self.lib.disco_last_error(self.ctx).decode()}')

    def close(self):
        if self.ctx:
            self.lib.disco_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # Every helper below that uploads returns the keep-alive beside the pointer, and its caller binds it to a local: a temporary DevBuf
    # frees its memory when the last reference goes, which must not happen before the library call that got the pointer has returned.
    def _out(self, out, shape, dtype, check):
        """An output the caller may own -> (array to return, device pointer, keep-alive): a fresh DevBuf of `shape` for None, else `out`
        itself after `check`: 'shape' (exactly `shape`) or 'size' (as many elements), both refusing a NumPy array, or 'any' (nothing is
        checked; a NumPy array is then uploaded to a temporary that receives the result in its place)."""
        if out is None:
            out = self.empty(shape, dtype)
        elif check == 'shape':
            assert tuple(out.shape) == tuple(shape) and not isinstance(out, np.ndarray)
        elif check == 'size':
            assert int(np.prod(tuple(out.shape))) == int(np.prod(shape, dtype=np.int64)) and not isinstance(out, np.ndarray)
        else:
            assert check == 'any', check
        return (out,) + self.to_device(out, dtype)

    def _alias(self, b, a, dev_a, dtype, none):
        """(pointer, keep-alive) of `b`, an argument that may be the object `a` already on the device as `dev_a`: the same object gives the
        same pointer with one upload (the C side picks its route by comparing the two pointers).  none='same': None stands for `a` as
        well (the whole-path masks); none='null': None reaches C as NULL."""
        assert none in ('same', 'null'), none
        if b is a or (b is None and none == 'same'):
            return dev_a
        return self.to_device(b, dtype)

    def _pencils(self, A, B):
        """The solvers' prologue: A, B (..., P, P) -> (shape, P, number of pencils, pointer of A, pointer of B, keep-alive)."""
        shape = tuple(A.shape)
        pa, ka = self.to_device(A, np.complex64)
        pb, kb = self.to_device(B, np.complex64)
        return shape, shape[-1], int(np.prod(shape[:-2], dtype=np.int64)), pa, pb, (ka, kb)

    def _selftest_pair(self, fn, inputs, dtype, shape):
        """fn(inputs (n,)..., n) -> (out_hw, out_ref), each `shape`: one instruction-level self-test of the library and its plain restatement."""
        dev = [self.to_device(a, dtype) for a in inputs]
        hw, ref = self.empty(shape, dtype), self.empty(shape, dtype)
        self._chk(fn(self.ctx, *(p for p, _ in dev), inputs[0].shape[0], hw.ptr, ref.ptr, self.stream))
        return hw, ref

    # ---- online / adaptive mode (primitives internal_formulas.py:84-103 and :56-73)
    def online_mwf(self, X, mask, Z=None, lambda_cor=0.95, mu=None, update_every=1, init_diag=1e-3, want_w=False):
        """Exponentially smoothed covariances + a filter update every `update_every` frames, causal in t.
        X (R,Kl,T,F,M), mask (R,Kl,T,F)[, Z (R,K,T,F) -> P = M+K-1]  ->  out (R,Kl,T,F)[, w_last (R,Kl,F,P)]."""
        P = self.M + (self.K - 1 if Z is not None else 0)
        px, kx = self.to_device(X, np.complex64)
        pz, kz = self.to_device(Z, np.complex64)
        pm, km = self.to_device(mask, np.float32)
        out = self.empty((self.R, self.Kl, self.T, self.F), np.complex64)
        w = self.empty((self.R, self.Kl, self.F, P), np.complex64) if want_w else None
        self._chk(self.lib.disco_online_mwf(self.ctx, px, pz, pm, P, lambda_cor, self.cfg.mu if mu is None else mu,
                                            update_every, init_diag, out.ptr, _ptr(w), self.stream))
        return (out, w) if want_w else out

    def tango_online(self, y, mask_z, mask_w=None, lambda_cor=0.95, update_every=1, init_diag=1e-3, want_z=True,
                     want_yf=True, out=None):
        """The two-step path in online mode: y (R,K,M,L), masks (R,K,T,F) -> out (R,K,L)[, z_y, yf (R,K,T,F)]."""
        py, ky = self.to_device(y, np.float32)
        pmz, kmz = self.to_device(mask_z, np.float32)
        pmw, kmw = self._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='same')
        out, po, ko = self._out(out, (self.R, self.K, self.Lsamp), np.float32, 'any')
        z = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_z else None
        yf = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_yf else None
        self._chk(self.lib.disco_tango_online(self.ctx, py, pmz, pmw, lambda_cor, update_every, init_diag, po, _ptr(z), _ptr(yf), None, 0,
                                              self.stream))
        return out, z, yf

    def online_mwf_ref(self, X, mask, S, N=None, Z=None, Zs=None, Zn=None, lambda_cor=0.95, mu=None, update_every=1, init_diag=1e-3,
                       want_w=False):
        """online_mwf with companions (disco_online_mwf_ref): S [, N] laid out as X and Zs [, Zn] as Z ride through the same per-frame
        filters as the mixture.  -> out, out_s[, out_n][, w_last]; out and w_last are those of online_mwf, bit for bit."""
        P = self.M + (self.K - 1 if Z is not None else 0)
        px, kx = self.to_device(X, np.complex64)
        pz, kz = self.to_device(Z, np.complex64)
        pm, km = self.to_device(mask, np.float32)
        out = self.empty((self.R, self.Kl, self.T, self.F), np.complex64)
        w = self.empty((self.R, self.Kl, self.F, P), np.complex64) if want_w else None
        pairs = [(S, Zs)] + ([(N, Zn)] if N is not None else [])
        comp = (L.DiscoOnlineCompanion * len(pairs))()
        keep, outs = [], []
        for i, (A, ZA) in enumerate(pairs):
            pa, ka = self.to_device(A, np.complex64)
            pza, kza = self.to_device(ZA, np.complex64)
            o = self.empty((self.R, self.Kl, self.T, self.F), np.complex64)
            comp[i].X, comp[i].Z, comp[i].out = pa, pza, o.ptr
            keep += [ka, kza]
            outs.append(o)
        self._chk(self.lib.disco_online_mwf_ref(self.ctx, px, pz, pm, P, lambda_cor, self.cfg.mu if mu is None else mu, update_every,
                                                init_diag, out.ptr, _ptr(w), comp, len(pairs), self.stream))
        return (out, *outs, w) if want_w else (out, *outs)

    def tango_online_reference(self, y, s, n, mask_z=None, mask_w=None, lambda_cor=0.95, update_every=1, init_diag=1e-3, want=None,
                               signals=False):
        """tango_reference's nine outputs in online mode, in ONE device-resident call (disco_tango_online_reference): y, s, n (R,K,M,L)
        float32; mask_z / mask_w (R,K,T,F) float32 or None (oracle TF masks of the engine's mask type).  Returns {name: DevBuf (R,K,T,F)}
        for the names in `want` (default: all nine); signals=True adds 'signals', a DevBuf (6,R,K,L): the inverse transforms of
        yf, sf, nf, z_y, z_s, z_n -- what results_io.batch_results takes as sh_t, sf_t, nf_t, szh_t, szf_t, nzf_t.  signals may also be a
        caller-owned device array of that shape (a torch tensor, which batch_results reads in place) to write them into."""
        names = [nm for nm in ('z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'yf', 'sf', 'nf', 'mask_w') if want is None or nm in want]
        py, ky = self.to_device(y, np.float32)
        ps, ks = self.to_device(s, np.float32)
        pn, kn = self.to_device(n, np.float32)
        pmz, kmz = self.to_device(mask_z, np.float32)
        pmw, kmw = self._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='null')         # None is the oracle mask, not mask_z
        bufs = {nm: self.empty((self.R, self.K, self.T, self.F), np.float32 if nm.startswith('mask') else np.complex64) for nm in names}
        outs = L.DiscoRefOutputs(**{nm: b.ptr for nm, b in bufs.items()})
        want_sig = signals is not False and signals is not None
        sig, psig, ksig = self._out(None if signals is True else signals, (6, self.R, self.K, self.Lsamp), np.float32, 'shape') if want_sig \
            else (None, None, None)
        self._chk(self.lib.disco_tango_online_reference(self.ctx, py, ps, pn, pmz, pmw, lambda_cor, update_every, init_diag, C.byref(outs),
                                                        psig, None, 0, self.stream))
        if want_sig:
            bufs['signals'] = sig
        return bufs

    def online_stream(self, lambda_cor=0.95, update_every=1, init_diag=1e-3):
        """A stream of the online two-step path (disco_tango_online_stream): `push(y_new, mask_z, mask_w=None, last=False)` consumes the
        next n_hops * hop samples of every channel, y_new (R, K, M, n_hops * hop), with the masks (R, K, n_new, F) of the frames it
        completes (n_new = n_hops + last), and returns the (R, K, n_out) output samples that became final.  The state block is owned by
        the returned object (caller-side memory as far as the library is concerned)."""
        return _OnlineStream(self, lambda_cor, update_every, init_diag)

    def mask_ivad(self, s_ref):
        """s_ref (n_sig, L) float32 (target image at channel 0) -> 'ivad' mask (n_sig, T, F)   [tango.py:217-221]"""
        n_sig, Ls = s_ref.shape
        assert Ls == self.Lsamp
        ps, ks = self.to_device(s_ref, np.float32)
        m = self.empty((n_sig, self.T, self.F), np.float32)
        self._chk(self.lib.disco_mask_ivad(self.ctx, ps, n_sig, m.ptr, self.stream))
        return m

    # ---- from reverberated sources to rooms (convolve_signals.py:102-115, 255-273; post_generator.py:99-115).  The conventions of
    # disco_amd.metrics: the last axis is time, the leading axes a batch; NumPy in gives NumPy out, a device array in gives a DevBuf
    @staticmethod
    def _lead_stops(stop, lead, L):
        """`stop` (None, a scalar, or an array broadcast over the leading axes) -> None or one int per flattened signal, each in [0, L]."""
        if stop is None:
            return None
        try:
            stops = np.ascontiguousarray(np.broadcast_to(np.asarray(stop), tuple(lead))).reshape(-1)
        except ValueError:
            raise ValueError(f'stop of shape {np.shape(stop)} does not broadcast to the leading axes {tuple(lead)}') from None
        if not np.issubdtype(stops.dtype, np.integer):
            raise ValueError(f'stop must hold integers, got {stops.dtype}')
        if np.any(stops < 0) or np.any(stops > L):
            raise ValueError(f'need 0 <= stop <= L = {L}: stop {stop}')
        return stops.astype(np.int32)

    def vad_samples(self, x, stop=None, win_len=512, win_hop=256, thr=0.001, rat=2):
        """x (..., L) float32 -> the per-sample VAD (..., L) of 0.0 / 1.0: vad_oracle_batch (sigproc_utils.py:12-55) of every signal
        (disco_vad_samples).  stop: signal i is processed as if sliced to stop[i] and run alone; zeros at and beyond it."""
        host = _on_host(x)
        if host:
            x = np.ascontiguousarray(x, dtype=np.float32)
        shape = tuple(int(v) for v in x.shape)
        lead, L = shape[:-1], shape[-1]
        n_sig = int(np.prod(lead, dtype=np.int64))
        stops = self._lead_stops(stop, lead, L)
        px, kx = self.to_device(x, np.float32)
        pst, kst = self.to_device(stops, np.int32)
        vad = self.empty(shape, np.float32)
        self._chk(self.lib.disco_vad_samples(self.ctx, px, n_sig, L, pst, win_len, win_hop, thr, rat, vad.ptr, self.stream))
        return vad.numpy() if host else vad

    def mix_scaled(self, s, n, gain, group=1, stop=None, want_n=True, want_y=True, n_out=None, y_out=None):
        """s (..., L) or None, n (..., Ln) with Ln <= L, gain: one float per `group` consecutive signals (a scalar serves all)
        -> (n_out, y_out), each (..., L) or None where not wanted: n_out = gain * n below min(Ln, stop), y_out = s + n_out below stop, exact
        zeros elsewhere (disco_mix_scaled); y_out - s == n_out bit for bit.  s = None: the scaled noise alone (want_y is then ignored).
        n_out / y_out: optional caller-owned device arrays to write into (n_out may be n itself when Ln == L); they are returned as given."""
        host = _on_host(n)
        if host:
            n = np.ascontiguousarray(n, dtype=np.float32)
        if s is not None and _on_host(s):
            s = np.ascontiguousarray(s, dtype=np.float32)
        nshape = tuple(int(v) for v in n.shape)
        lead, Ln = nshape[:-1], nshape[-1]
        L = Ln if s is None else int(s.shape[-1])
        if s is not None and tuple(int(v) for v in s.shape[:-1]) != lead:
            raise ValueError(f's and n must share their leading axes: {tuple(s.shape)} and {nshape}')
        if Ln > L:
            raise ValueError(f'the noise ({Ln} samples) is longer than the signal ({L})')
        want_y = (want_y or y_out is not None) and s is not None
        want_n = want_n or n_out is not None
        if not (want_n or want_y):
            raise ValueError('nothing asked for: want_n or want_y (with s given)')
        n_sig = int(np.prod(lead, dtype=np.int64))
        if group < 1 or n_sig % group:
            raise ValueError(f'{n_sig} signals are no multiple of group = {group}')
        if _on_host(gain):
            try:
                gain = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=np.float32).reshape(-1), (n_sig // group,)))
            except ValueError:
                raise ValueError(f'gain of shape {np.shape(gain)} does not give one value per {group} of {n_sig} signals') from None
        stops = self._lead_stops(stop, lead, L)
        pn, kn = self.to_device(n, np.float32)
        ps, ks = self.to_device(s if want_y else None, np.float32)
        pg, kg = self.to_device(gain, np.float32)
        pst, kst = self.to_device(stops, np.int32)
        pno = pyo = None
        fresh_n, fresh_y = n_out is None, y_out is None                      # a fresh output follows the container of n
        if want_n:
            n_out, pno, kno = self._out(n_out, lead + (L,), np.float32, 'size')
        if want_y:
            y_out, pyo, kyo = self._out(y_out, lead + (L,), np.float32, 'size')
        self._chk(self.lib.disco_mix_scaled(self.ctx, ps, pn, n_sig, L, Ln, pg, group, pst, pno, pyo, self.stream))
        return ((n_out.numpy() if host and fresh_n else n_out) if want_n else None,
                (y_out.numpy() if host and fresh_y else y_out) if want_y else None)

    def source_mix(self, images, target, stop=None, want_y=True, want_s=True, want_n=True):
        """images (S, ..., n_mic, L), source-major; target: n_mic ints, target[c] in [0, S) the talker channel c listens to
        -> (y, s, n), each (..., n_mic, L) or None where not wanted: y = ((img_0 + img_1) + img_2) + ..., s = img_target, n = the sum of
        the others in ascending order -- float32 additions in exactly that order, one pass over the images (disco_source_mix).  stop:
        None, a scalar, or an array broadcast over (..., n_mic): exact zeros at and beyond it, where nothing is read.  2 <= S <= 8."""
        host = _on_host(images)
        if host:
            images = np.ascontiguousarray(images, dtype=np.float32)
        shape = tuple(int(v) for v in images.shape)
        if len(shape) < 3:
            raise ValueError(f'images must be (S, ..., n_mic, L): {shape}')
        S, lead, L = shape[0], shape[1:-1], shape[-1]
        n_mic = lead[-1]
        tgt = np.asarray(target).reshape(-1)
        if tgt.shape != (n_mic,) or not np.issubdtype(tgt.dtype, np.integer):
            raise ValueError(f'target must hold one integer per channel ({n_mic}): {np.shape(target)}, {tgt.dtype}')
        if not (want_y or want_s or want_n):
            raise ValueError('nothing asked for: want_y, want_s or want_n')
        tgt = np.ascontiguousarray(tgt, dtype=np.int32)
        n_row = int(np.prod(lead, dtype=np.int64))
        stops = self._lead_stops(stop, lead, L)
        pi, ki = self.to_device(images, np.float32)
        pst, kst = self.to_device(stops, np.int32)
        outs = [self.empty(lead + (L,), np.float32) if w else None for w in (want_y, want_s, want_n)]
        self._chk(self.lib.disco_source_mix(self.ctx, pi, S, n_row, L, tgt.ctypes.data, n_mic, pst, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                            self.stream))
        return tuple(o.numpy() if host and o is not None else o for o in outs)

    # ---- dry sources (dataset_utils/signal_setups.py:42-138): the same conventions
    @staticmethod
    def _lead_values(v, lead, dtype, name):
        """One value per flattened signal from None (-> None: the C side's default), a scalar or an array broadcast over the leading axes."""
        if v is None:
            return None
        try:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v), tuple(lead)), dtype=dtype).reshape(-1)
        except ValueError:
            raise ValueError(f'{name} of shape {np.shape(v)} does not broadcast to the leading axes {tuple(lead)}') from None

    def noise_from_signal(self, x, phase, stop=None, n_fft=None, max_workspace=1 << 30, out=None):
        """x (..., L) float32, phase (..., n_fft / 2 + 1) float32 in turns, [0, 1) -> (..., L): irfft(|rfft(x_i[:stop_i], n_fft)| *
        exp(2 pi i phase_i), n_fft)[:stop_i], zeros at and beyond stop_i (disco_noise_from_signal; sigproc_utils.py:257-279 with the
        phases given).  n_fft: a power of two from 2^10 to 2^22, by default the smallest that holds the longest signal.  The batch is
        walked in chunks of signals so that the transform's workspace in the context (8 n_fft bytes per signal) stays under
        max_workspace bytes; one signal always goes.  out: an optional caller-owned device array of as many elements, returned as given."""
        from .math_utils import next_pow_2
        host = _on_host(x)
        if host:
            x = np.ascontiguousarray(x, dtype=np.float32)
        shape = tuple(int(v) for v in x.shape)
        lead, L = shape[:-1], shape[-1]
        n_sig = int(np.prod(lead, dtype=np.int64))
        stops = self._lead_stops(stop, lead, L)
        longest = L if stops is None else int(stops.max(initial=0))
        n_fft = max(next_pow_2(max(longest, 1)), 1024) if n_fft is None else int(n_fft)
        if n_fft < 1 or n_fft & (n_fft - 1):
            raise ValueError(f'n_fft must be a power of two: {n_fft}')
        if longest > n_fft:
            raise ValueError(f'a signal of {longest} samples does not fit n_fft = {n_fft}')
        if _on_host(phase):
            phase = np.ascontiguousarray(phase, dtype=np.float32)
        if tuple(int(v) for v in phase.shape) != lead + (n_fft // 2 + 1,):
            raise ValueError(f'phase must be {lead + (n_fft // 2 + 1,)} for n_fft = {n_fft}: {tuple(phase.shape)}')
        px, kx = self.to_device(x, np.float32)
        pp, kp = self.to_device(phase, np.float32)
        pst, kst = self.to_device(stops, np.int32)
        fresh = out is None
        out, po, ko = self._out(out, shape, np.float32, 'size')
        step = max(1, int(max_workspace) // (8 * n_fft))
        for i0 in range(0, n_sig, step):
            m = min(step, n_sig - i0)
            self._chk(self.lib.disco_noise_from_signal(self.ctx, px + 4 * i0 * L, m, L, None if pst is None else pst + 4 * i0, n_fft,
                                                       pp + 4 * i0 * (n_fft // 2 + 1), po + 4 * i0 * L, self.stream))
        return out.numpy() if host and fresh else out

    def affine_segment(self, x, stop=None, start=None, count=None, mean=None, gain=None, lead=0, out_len=None, out=None):
        """x (..., L) float32 -> (..., out_len), out_len = lead + L by default:
            out[i, lead + t] = float32((float64(x[i, (start_i + t) % L_i]) - mean_i) * gain_i)    for 0 <= t < min(count_i, out_len - lead)
        and exact zeros elsewhere (disco_affine_segment), L_i = stop_i.  stop, start, count (integers), mean, gain (float64): None (L,
        0, L_i, 0, 1), a scalar, or an array broadcast over the leading axes.  out: an optional caller-owned device array of as many
        elements, returned as given."""
        host = _on_host(x)
        if host:
            x = np.ascontiguousarray(x, dtype=np.float32)
        shape = tuple(int(v) for v in x.shape)
        lead_axes, L = shape[:-1], shape[-1]
        n_sig = int(np.prod(lead_axes, dtype=np.int64))
        lead = int(lead)
        out_len = lead + L if out_len is None else int(out_len)
        if not 0 <= lead <= out_len:
            raise ValueError(f'need 0 <= lead <= out_len: lead {lead}, out_len {out_len}')
        stops = self._lead_stops(stop, lead_axes, L)
        for name, v in (('start', start), ('count', count)):
            if v is not None and not np.issubdtype(np.asarray(v).dtype, np.integer):
                raise ValueError(f'{name} must hold integers, got {np.asarray(v).dtype}')
        px, kx = self.to_device(x, np.float32)
        pst, kst = self.to_device(stops, np.int32)
        psa, ksa = self.to_device(self._lead_values(start, lead_axes, np.int32, 'start'), np.int32)
        pc, kc = self.to_device(self._lead_values(count, lead_axes, np.int32, 'count'), np.int32)
        pm, km = self.to_device(self._lead_values(mean, lead_axes, np.float64, 'mean'), np.float64)
        pg, kg = self.to_device(self._lead_values(gain, lead_axes, np.float64, 'gain'), np.float64)
        fresh = out is None
        out, po, ko = self._out(out, lead_axes + (out_len,), np.float32, 'size')
        self._chk(self.lib.disco_affine_segment(self.ctx, px, n_sig, L, pst, psa, pc, pm, pg, lead, po, out_len, self.stream))
        return out.numpy() if host and fresh else out

    # ---- the step before the path (gen_disco/convolve_signals.py:160-163)
    def rir_convolve(self, dry, rir, out_len=None):
        """dry (n_sig, Ld), rir (n_sig, n_ch, Lh) float32 -> (n_sig, n_ch, out_len) = np.convolve(dry_i, rir_ic)[:out_len]."""
        n_sig, Ld = dry.shape
        n_sig2, n_ch, Lh = rir.shape
        assert n_sig == n_sig2
        out_len = Ld if out_len is None else out_len
        pd, kd = self.to_device(dry, np.float32)
        pr, kr = self.to_device(rir, np.float32)
        out = self.empty((n_sig, n_ch, out_len), np.float32)
        self._chk(self.lib.disco_rir_convolve(self.ctx, pd, pr, n_sig, n_ch, Ld, Lh, out.ptr, out_len, self.stream))
        return out

    def ism_rir(self, room_dims, absorption, src, mic, max_order=20, fs=16000.0, c_sound=343.0, rir_len=4096):
        """Shoebox image-source RIRs: room_dims (n_room, 3), absorption (n_room,), src (n_room, S, 3), mic (n_room, Q, 3)
        -> rir (n_room, S, Q, rir_len)   [pra.ShoeBox(...).compute_rir(), convolve_signals.py:243-246, 94-95]"""
        n_room = room_dims.shape[0]
        S, Q = src.shape[1], mic.shape[1]
        pd, kd = self.to_device(room_dims, np.float32)
        pa, ka = self.to_device(absorption, np.float32)
        ps, ks = self.to_device(src, np.float32)
        pm, km = self.to_device(mic, np.float32)
        out = self.empty((n_room, S, Q, rir_len), np.float32)
        self._chk(self.lib.disco_ism_rir(self.ctx, pd, pa, ps, pm, n_room, S, Q, max_order, fs, c_sound, out.ptr, rir_len, self.stream))
        return out

    # ---- evaluation metrics (disco_theque/metrics.py)
    def _span_stops(self, stop, n, L, start):
        """`stop` of a metric call -> (scalar stop, None) for None / a scalar, or (None, (device pointer, keep-alive)) for an (n,) array:
        one stop per signal, validated on the host and uploaded once (the `_spans` entry points)."""
        if stop is None or not np.ndim(stop):
            return (L if stop is None else int(stop)), None
        stops = np.asarray(stop)
        if stops.shape != (n,):
            raise ValueError(f'stop must be None, a scalar or an ({n},) array, one entry per signal: got shape {stops.shape}')
        if not np.issubdtype(stops.dtype, np.integer):
            raise ValueError(f'stop must hold integers, got {stops.dtype}')
        return None, self._upload_stops(stops, L, start, stop)

    def _upload_stops(self, stops, L, start, given):
        """The range check and the upload of an (n,) integer array of stops -> (device pointer, keep-alive); `given` is what the error shows."""
        if int(start) < 0 or np.any(stops < start) or np.any(stops > L):
            raise ValueError(f'need 0 <= start <= stop <= L = {L}: start {start}, stop {given}')
        return self.to_device(np.ascontiguousarray(stops, dtype=np.int32), np.int32)

    def _span_stops_dev(self, stop, n, L, start, dialect):
        """`stop` of an entry point that takes one stop per signal or NULL -> (device pointer, keep-alive), or (None, None) for None, when
        `start` alone is checked.  dialect 'each' (bss_estimates): a scalar is repeated n times, an array goes through `_span_stops`;
        'broadcast' (stoi): whatever np.broadcast_to takes to (n,), converted to int64 first, so a float is truncated, not refused."""
        if stop is None:
            if not 0 <= int(start) <= L:
                raise ValueError(f'need 0 <= start <= L = {L}: start {start}')
            return None, None
        if dialect == 'broadcast':
            return self._upload_stops(np.broadcast_to(np.asarray(stop, dtype=np.int64), (n,)), L, start, stop)
        assert dialect == 'each', dialect
        return self._span_stops(stop if np.ndim(stop) else np.full((n,), int(stop), dtype=np.int64), n, L, start)[1]

    def _chunk_plan(self, n, ws_bytes, budget_bytes, default_budget, probe, name):
        """A batch of n items walked under a workspace budget -> (items per chunk, workspace DevBuf): ws_bytes(k) is the library's size for
        k items, at least one item goes per chunk.  ws_bytes(1) == 0 means a shape outside the supported range: `probe()` calls the
        entry point with NULLs so that the library names the limit (nothing is launched), then DiscoError."""
        per_item = int(ws_bytes(1))
        if per_item == 0:
            self._chk(probe())
            raise DiscoError(f'{name}: unsupported shape')
        budget = default_budget if budget_bytes is None else int(budget_bytes)
        step = max(1, min(n, budget // per_item))
        return step, self.empty((int(ws_bytes(step)) // 8 + 1,), np.float64)

    def _chunks(self, n, step, *inputs):
        """The walk itself: yields (i0, n_chunk, pointer...) with one float32 pointer per (array, elements per item) in `inputs`.  A NumPy
        array is sliced and uploaded chunk by chunk (the upload stays referenced until the next chunk is asked for); a device-resident
        one is read in place, its pointer stepped."""
        host = [isinstance(a, np.ndarray) for a, _ in inputs]
        base = [None if h else self.to_device(a, np.float32) for (a, _), h in zip(inputs, host)]
        for i0 in range(0, n, step):
            m = min(step, n - i0)
            dev = [self.to_device(a[i0:i0 + m], np.float32) if h else (b[0] + 4 * i0 * per, b[1]) for (a, per), h, b in zip(inputs, host, base)]
            yield (i0, m) + tuple(p for p, _ in dev)

    def pair_stats(self, a, b, start=0, stop=None):
        """a, b (n_sig, L) float32 -> (n_sig, 8) float64 moments of a[:, start:stop], b[:, start:stop]
        {#(a!=0), sum a, sum a^2, #(b!=0), sum b, sum b^2, sum ab, n}.  stop: None (L), a scalar, or an (n_sig,) array -- signal i is
        then scored over [start, stop[i]) and nothing at or beyond stop[i] is read (disco_pair_stats_spans)."""
        n_sig, L = a.shape
        stop, dstop = self._span_stops(stop, n_sig, L, start)
        pa, ka = self.to_device(a, np.float32)
        pb, kb = self._alias(b, a, (pa, ka), np.float32, none='null')
        st = self.empty((n_sig, 8), np.float64)
        if dstop is not None:
            self._chk(self.lib.disco_pair_stats_spans(self.ctx, pa, pb, n_sig, L, start, dstop[0], st.ptr, self.stream))
        else:
            self._chk(self.lib.disco_pair_stats(self.ctx, pa, pb, n_sig, L, start, stop, st.ptr, self.stream))
        return st

    def band_stats(self, x, b, a, start=0, stop=None, gate=None):
        """x (n_sig, L) float32; b, a (n_bands, 9) float64 -> (n_sig, n_bands, 3) float64 {#(y!=0), sum y, sum y^2} of
        y = lfilter(b_j, a_j, x[:, start:stop]); gate (n_sig, L) float32: the samples with gate != 0 instead of those with y != 0.
        stop: None (L), a scalar, or an (n_sig,) array -- signal i is filtered and scored over [start, stop[i]) (disco_band_stats_spans)."""
        n_sig, L = x.shape
        stop, dstop = self._span_stops(stop, n_sig, L, start)
        b = np.ascontiguousarray(b, np.float64)
        a = np.ascontiguousarray(a, np.float64)
        assert b.shape == a.shape and b.shape[1] == 9, 'order-4 band-pass (9 coefficients per polynomial) expected'
        px, kx = self.to_device(x, np.float32)
        pb, kb = self.to_device(b, np.float64)
        pa, ka = self.to_device(a, np.float64)
        st = self.empty((n_sig, b.shape[0], 3), np.float64)
        pg = kg = None
        if gate is not None:
            assert tuple(gate.shape) == (n_sig, L), 'the gate is indexed like the signals'
            pg, kg = self.to_device(gate, np.float32)
        if dstop is not None:
            self._chk(self.lib.disco_band_stats_spans(self.ctx, px, pg, n_sig, L, start, dstop[0], pb, pa, b.shape[0], st.ptr, self.stream))
        elif gate is not None:
            self._chk(self.lib.disco_band_stats_gated(self.ctx, px, pg, n_sig, L, start, stop, pb, pa, b.shape[0], st.ptr, self.stream))
        else:
            self._chk(self.lib.disco_band_stats(self.ctx, px, n_sig, L, start, stop, pb, pa, b.shape[0], st.ptr, self.stream))
        return st

    def seg_snr(self, s, n, win_len, win_hop, vad=None, start=0, stop=None, lo_db=-15.0, hi_db=25.0):
        """s, n (n_sig, L) float32, vad (n_sig, L) float32 or None -> (n_sig, 4) float64 {sum g v, sum g, N_w, #windows at a clip bound} of
        the segmental SNR over [start, stop) (disco_seg_snr): v the clipped window level ratio in dB, g = 1 or vad[:, start + m win_hop].
        stop: None (L), a scalar, or an (n_sig,) array -- nothing at or beyond stop[i] is read."""
        if len(s.shape) != 2 or tuple(s.shape) != tuple(n.shape):
            raise ValueError(f's and n must both be (n_sig, L): {tuple(s.shape)} and {tuple(n.shape)}')
        n_sig, L = (int(v) for v in s.shape)
        if vad is not None and tuple(vad.shape) != (n_sig, L):
            raise ValueError(f'the VAD is indexed like the signals, {(n_sig, L)}: {tuple(vad.shape)}')
        pst, kst = self._span_stops_dev(stop, n_sig, L, start, 'each')
        ps, ks = self.to_device(s, np.float32)
        pn, kn = self._alias(n, s, (ps, ks), np.float32, none='null')
        pv, kv = self.to_device(vad, np.float32)
        out = self.empty((n_sig, 4), np.float64)
        self._chk(self.lib.disco_seg_snr(self.ctx, ps, pn, pv, n_sig, L, start, pst, win_len, win_hop, lo_db, hi_db, out.ptr, self.stream))
        return out

    # ---- how reverberant a room came out (metrics.py:176-208)
    def rir_split(self, rir, n_direct):
        """rir (..., rir_len) float32 -> (split (...,) int32, energy (..., 2) float64) as DevBufs: split = min(argmax + n_direct, rir_len),
        energy = {sum rir[:split]^2, sum rir[split:]^2}  (disco_rir_split)."""
        shape = tuple(int(v) for v in rir.shape)
        n_rir = int(np.prod(shape[:-1], dtype=np.int64))
        pr, kr = self.to_device(rir, np.float32)
        split, energy = self.empty(shape[:-1], np.int32), self.empty(shape[:-1] + (2,), np.float64)
        self._chk(self.lib.disco_rir_split(self.ctx, pr, n_rir, shape[-1], int(n_direct), split.ptr, energy.ptr, self.stream))
        return split, energy

    def reverb_energies(self, dry, rir, split):
        """dry (n_sig, Ld), rir (n_sig, n_ch, rir_len) float32, split (n_sig, n_ch) int32 -> (n_sig, n_ch, 2) float64
        {sum (dry * rir[:split])^2, sum (dry * rir[split:])^2} over the full convolutions, neither of which is written to memory
        (disco_reverb_energies)."""
        if len(dry.shape) != 2 or len(rir.shape) != 3 or int(rir.shape[0]) != int(dry.shape[0]):
            raise ValueError(f'dry must be (n_sig, Ld) and rir (n_sig, n_ch, rir_len): {tuple(dry.shape)} and {tuple(rir.shape)}')
        n_sig, Ld = (int(v) for v in dry.shape)
        n_ch, Lh = int(rir.shape[1]), int(rir.shape[2])
        if tuple(int(v) for v in split.shape) != (n_sig, n_ch):
            raise ValueError(f'split must be {(n_sig, n_ch)}: {tuple(split.shape)}')
        pd, kd = self.to_device(dry, np.float32)
        pr, kr = self.to_device(rir, np.float32)
        psp, ksp = self.to_device(split, np.int32)
        energy = self.empty((n_sig, n_ch, 2), np.float64)
        self._chk(self.lib.disco_reverb_energies(self.ctx, pd, pr, psp, n_sig, n_ch, Ld, Lh, energy.ptr, self.stream))
        return energy

    def lag_corr(self, a, b, lag_lo, lag_hi, start=0, stop=None):
        """a, b (n_pair, L) float32 -> (n_pair, lag_hi - lag_lo + 1) float64: c[i][t - lag_lo] = sum_n a[i][n] b[i][n + t] over the n with
        n and n + t inside [start, stop); lags within +-511  (disco_lag_corr).  stop: None (L), a scalar, or an (n_pair,) array -- pair i
        then counts as zero outside [start, stop[i]) and is not read there (disco_lag_corr_spans)."""
        if len(a.shape) != 2 or tuple(a.shape) != tuple(b.shape):
            raise ValueError(f'a and b must both be (n_pair, L): {tuple(a.shape)} and {tuple(b.shape)}')
        n_pair, L = (int(v) for v in a.shape)
        stop, dstop = self._span_stops(stop, n_pair, L, start)
        nlag = int(lag_hi) - int(lag_lo) + 1
        pa, ka = self.to_device(a, np.float32)
        pb, kb = self._alias(b, a, (pa, ka), np.float32, none='null')
        wsb = int(self.lib.disco_lag_corr_workspace_bytes(self.ctx, n_pair, L, max(nlag, 1)))
        ws = self.empty((max(wsb, 8) // 8,), np.float64)
        out = self.empty((n_pair, max(nlag, 1)), np.float64)
        if dstop is not None:
            self._chk(self.lib.disco_lag_corr_spans(self.ctx, pa, pb, n_pair, L, start, dstop[0], lag_lo, lag_hi, out.ptr, ws.ptr, ws.nbytes,
                                                    self.stream))
        else:
            self._chk(self.lib.disco_lag_corr(self.ctx, pa, pb, n_pair, L, start, stop, lag_lo, lag_hi, out.ptr, ws.ptr, ws.nbytes, self.stream))
        return out

    BSS_WORKSPACE_BUDGET = 1 << 30      # bytes of factor / correlation workspace one disco_bss_eval call of Engine.bss_eval may take

    def bss_eval(self, refs, ests, start=0, stop=None, flen=512, all_pairs=False, budget_bytes=None):
        """BSS-eval energies (disco_bss_eval): refs (n_set, nsrc, L), ests (n_set, n_est, nsrc, L) float32 -> (energies, status), NumPy:
        energies (n_set, n_est, nsrc, 4), estimate i against source i, or (n_set, n_est, nsrc, nsrc, 4) with all_pairs, estimate i against
        source j -- each {p_j, p_all, ee, status}; status (n_set,) int32, non-zero where the set's Gram matrix is singular to working
        precision (its energies are NaN).  A large batch is walked in chunks of sets whose workspace stays under `budget_bytes` (default
        BSS_WORKSPACE_BUDGET; 10 MB of factors per two-source set at flen 512, so about 100 sets per chunk); the chunking does not
        change a bit of the result.  NumPy inputs are copied chunk by chunk; device-resident tensors / DevBufs are read in place.
        stop: None (L), a scalar, or an (n_set,) array -- set i, references and estimates, is then scored over [start, stop[i]) and not
        read outside it (disco_bss_eval_spans); the array is uploaded once and walked along with the sets."""
        rs, es = tuple(int(v) for v in refs.shape), tuple(int(v) for v in ests.shape)
        if len(rs) != 3 or len(es) != 4 or es[0] != rs[0] or es[2:] != rs[1:]:
            raise ValueError(f'refs must be (n_set, nsrc, L) and ests (n_set, n_est, nsrc, L): {rs} and {es}')
        n_set, nsrc, L = rs
        n_est = es[1]
        if min(n_set, nsrc, L, n_est) < 1:
            raise ValueError(f'empty batch: refs {rs}, ests {es}')
        stop, dstop = self._span_stops(stop, n_set, L, start)
        flen = int(flen)
        step, ws = self._chunk_plan(
            n_set, lambda k: self.lib.disco_bss_workspace_bytes(self.ctx, k, nsrc, flen, L), budget_bytes, self.BSS_WORKSPACE_BUDGET,
            lambda: self.lib.disco_bss_eval(self.ctx, None, None, n_set, nsrc, n_est, L, start, L if stop is None else stop, flen, int(all_pairs),
                                            None, None, None, 0, self.stream), 'disco_bss_eval')
        oshape = (nsrc, nsrc, 4) if all_pairs else (nsrc, 4)
        energies = np.empty((n_set, n_est) + oshape, np.float64)
        status = np.empty((n_set,), np.int32)
        for i0, n, pr, pe in self._chunks(n_set, step, (refs, nsrc * L), (ests, n_est * nsrc * L)):
            out = self.empty((n, n_est) + oshape, np.float64)
            st = self.empty((n,), np.int32)
            if dstop is not None:
                self._chk(self.lib.disco_bss_eval_spans(self.ctx, pr, pe, n, nsrc, n_est, L, start, dstop[0] + 4 * i0, flen, int(all_pairs), out.ptr,
                                                        st.ptr, ws.ptr, ws.nbytes, self.stream))
            else:
                self._chk(self.lib.disco_bss_eval(self.ctx, pr, pe, n, nsrc, n_est, L, start, stop, flen, int(all_pairs), out.ptr, st.ptr, ws.ptr,
                                                  ws.nbytes, self.stream))
            energies[i0:i0 + n] = out.numpy()
            status[i0:i0 + n] = st.numpy()
        return energies, status

    def bss_estimates(self, y, sh, szh, start=0, stop=None, out=None):
        """The three estimate sets tango.py:547-549 scores per node (disco_bss_estimates): y, sh, szh (n_sig, L) float32 -- mixture, step-2
        output, step-1 output -> DevBuf (n_sig, 3, 2, L) float32 = {sh, y - sh}, {szh, y - szh}, {y, y - sh}, each difference formed in
        float64 and rounded to float32 once; exact zeros outside [start, stop[i]), where nothing is read.  stop: None (L), a scalar or an
        (n_sig,) array.  out: optional caller-owned device array of n_sig * 6 * L float32 to write into."""
        shp = tuple(int(v) for v in y.shape)
        if len(shp) != 2 or tuple(int(v) for v in sh.shape) != shp or tuple(int(v) for v in szh.shape) != shp:
            raise ValueError(f'y, sh and szh must all be (n_sig, L): {shp}, {tuple(sh.shape)} and {tuple(szh.shape)}')
        n_sig, L = shp
        if min(n_sig, L) < 1:
            raise ValueError(f'empty batch: {shp}')
        pstop, kstop = self._span_stops_dev(stop, n_sig, L, start, 'each')
        py, ky = self.to_device(y, np.float32)
        ps, ks = self.to_device(sh, np.float32)
        pz, kz = self.to_device(szh, np.float32)
        out, po, ko = self._out(out, (n_sig, 3, 2, L), np.float32, 'size')
        self._chk(self.lib.disco_bss_estimates(self.ctx, py, ps, pz, n_sig, L, int(start), pstop, po, self.stream))
        return out

    STOI_WORKSPACE_BUDGET = 1 << 30     # bytes of workspace one disco_stoi call of Engine.stoi may take

    def stoi(self, x, y, fs_sig, start=0, stop=None, budget_bytes=None, want_kept=False):
        """STOI (disco_stoi, csrc/k_stoi.h): x clean, y processed, both (n_pair, L) float32 at `fs_sig` Hz -> (d, status), NumPy: d (n_pair,)
        float64, status (n_pair,) int32 -- 0 scored, 1 fewer than 30 frames after the silent-frame removal (d = 1e-5), 2 the span gives no
        frame at all (d = NaN).  Pair i is scored over [start, stop[i]): `stop` is None (L), a scalar, or an (n_pair,) array, so that
        rooms of different clip lengths score as if each ran alone.  A large batch is walked in chunks of pairs whose workspace stays
        under `budget_bytes` (default STOI_WORKSPACE_BUDGET; the resampled signals are about 0.72 MB per 9-s pair); the chunking does
        not change a bit of the result.  NumPy inputs are copied chunk by chunk; device-resident tensors / DevBufs are read in place.
        want_kept: also return the number of frames kept per pair, (n_pair,) int64."""
        return self._stoi_call('disco_stoi', x, y, fs_sig, start, stop, budget_bytes, want_kept)

    def estoi(self, x, y, fs_sig, start=0, stop=None, budget_bytes=None, want_kept=False):
        """ESTOI, the extended STOI of Jensen & Taal 2016 (disco_estoi, csrc/k_estoi.h): the arguments, the chunk walk under
        STOI_WORKSPACE_BUDGET, the status values and the returns of `stoi`.  Resampling, silent-frame removal and the 15 third-octave
        envelopes are STOI's; every 15 x 30 segment is then normalised by rows (mean and norm over the 30 frames) and by columns (over the
        15 bands) without clipping, and d is the mean of the column correlations, in float64.  pystoi (extended=True) adds EPS randn
        before each normalisation so that it never divides by zero; that jitter is not reproduced (it moves d by some 1e-15 on the
        cases of tests/estoi_checks.py): the result is deterministic, and a row or column whose centred norm is exactly 0 contributes 0."""
        return self._stoi_call('disco_estoi', x, y, fs_sig, start, stop, budget_bytes, want_kept)

    def estoi_bands(self, X, Y, frames=None):
        """The last stage of ESTOI alone (disco_estoi_bands) on third-octave envelopes computed elsewhere: X clean, Y processed, both
        (n_pair, 15, tmax) float32 -> (d, status), NumPy: d (n_pair,) float64, status (n_pair,) int32 -- 0 scored, 1 fewer than 30 frames
        (d = 1e-5).  frames: None (tmax frames for every pair) or (n_pair,) integers 0 <= frames[i] <= tmax; nothing at or beyond a
        pair's count is read.  A pair has the same bits alone and in any batch."""
        xs, ys = tuple(int(v) for v in X.shape), tuple(int(v) for v in Y.shape)
        if len(xs) != 3 or xs != ys or xs[1] != 15:
            raise ValueError(f'X and Y must both be (n_pair, 15, tmax): {xs} and {ys}')
        n_pair, _, tmax = xs
        if min(n_pair, tmax) < 1:
            raise ValueError(f'empty batch: {xs}')
        pf = kf = None
        if frames is not None:
            fr = np.asarray(frames)
            if fr.shape != (n_pair,) or not np.issubdtype(fr.dtype, np.integer) or np.any(fr < 0) or np.any(fr > tmax):
                raise ValueError(f'frames must hold one integer in [0, {tmax}] per pair, shape ({n_pair},): got {fr.dtype} {fr.shape} {frames}')
            pf, kf = self.to_device(np.ascontiguousarray(fr, dtype=np.int32), np.int32)
        px, kx = self.to_device(X, np.float32)
        py, ky = self.to_device(Y, np.float32)
        n_chunk = -(-max(tmax - 29, 0) // L.ESTOI_SEGS)
        ws = self.empty((n_pair * n_chunk + 1,), np.float64)
        out = self.empty((n_pair, 2), np.float64)
        st = self.empty((n_pair,), np.int32)
        self._chk(self.lib.disco_estoi_bands(self.ctx, px, py, n_pair, tmax, pf, out.ptr, st.ptr, ws.ptr, ws.nbytes, self.stream))
        return out.numpy()[:, 0].copy(), st.numpy()

    def _stoi_call(self, name, x, y, fs_sig, start, stop, budget_bytes, want_kept):
        """`stoi` and `estoi`: entry point `name` and its `<name>_workspace_bytes` walked over the pairs."""
        entry, ws_bytes = getattr(self.lib, name), getattr(self.lib, name + '_workspace_bytes')
        xs, ys = tuple(int(v) for v in x.shape), tuple(int(v) for v in y.shape)
        if len(xs) != 2 or xs != ys:
            raise ValueError(f'x and y must both be (n_pair, L): {xs} and {ys}')
        n_pair, L = xs
        if min(n_pair, L) < 1:
            raise ValueError(f'empty batch: {xs}')
        p, q, taps = stoi_resample_taps(fs_sig)
        start = int(start)
        pstop, kstop = self._span_stops_dev(stop, n_pair, L, start, 'broadcast')
        ptaps = None
        if p != q:
            if not hasattr(self, '_stoi_taps'):
                self._stoi_taps = {}
            if (p, q) not in self._stoi_taps:
                self._stoi_taps[p, q] = self.to_device(taps, np.float64)
            ptaps = self._stoi_taps[p, q][0]
        n_taps = len(taps)
        step, ws = self._chunk_plan(
            n_pair, lambda k: ws_bytes(self.ctx, k, L, p, q, n_taps), budget_bytes, self.STOI_WORKSPACE_BUDGET,
            lambda: entry(self.ctx, None, None, n_pair, L, start, None, p, q, None, n_taps, None, None, None, 0, self.stream), name)
        d = np.empty((n_pair,), np.float64)
        kept = np.empty((n_pair,), np.int64)
        status = np.empty((n_pair,), np.int32)
        for i0, n, px, py in self._chunks(n_pair, step, (x, L), (y, L)):
            out = self.empty((n, 2), np.float64)
            st = self.empty((n,), np.int32)
            self._chk(entry(self.ctx, px, py, n, L, start, None if pstop is None else pstop + 4 * i0, p, q, ptaps, n_taps, out.ptr, st.ptr, ws.ptr,
                            ws.nbytes, self.stream))
            o = out.numpy()
            d[i0:i0 + n] = o[:, 0]
            kept[i0:i0 + n] = o[:, 1].astype(np.int64)
            status[i0:i0 + n] = st.numpy()
        return (d, status, kept) if want_kept else (d, status)

    def selftest_pk(self, a, b, c):
        """a, b, c (n,) complex64 -> (out_hw, out_ref), each (n, 23) complex64: the packed complex operations of
        csrc/pk.h through the v_pk_* instruction forms and through their C++ statement (include/disco_hip.h)."""
        return self._selftest_pair(self.lib.disco_selftest_pk, (a, b, c), np.complex64, (a.shape[0], 23))

    def selftest_dpp(self, a, b):
        """a, b (n,) complex128, n a multiple of 64 -> (out_hw, out_ref), each (n, 8) complex128: the float64 DPP row-broadcast forms of
        csrc/dpp64.h through their instructions and through __shfl + plain statements (include/disco_hip.h)."""
        return self._selftest_pair(self.lib.disco_selftest_dpp, (a, b), np.complex128, (a.shape[0], 8))

    def selftest_room(self, src):
        """src (n,) float32, n a multiple of 256 -> (out_hw, out_ref), each (n // 4, 6) float32: the LDS-DMA loads and permlane swaps of
        csrc/k_room.h through their instructions and through plain statements (include/disco_hip.h)."""
        return self._selftest_pair(self.lib.disco_selftest_room, (src,), np.float32, (src.shape[0] // 4, 6))

    STAGED_ROUTES = {1: 'room', 2: 'split_skiploc', 3: 'whole'}

    def selftest_staged_step2(self, X, mask, w_loc, store_z=True, z=None):
        """Step 1 on the caller's X (R,K,T,F,M) / mask (R,K,T,F), then the staged step 2 of the whole-path calls with filters w_loc
        (R,K,F,M) (include/disco_hip.h) -> (z (R,K,T,F), route name); the pencil stays pending for `gevd_mwf_r1_pending(M+K-1)` and
        `selftest_pending_matrices`.  z: optional caller-owned device array to write into."""
        px, kx = self.to_device(X, np.complex64)
        pm, km = self.to_device(mask, np.float32)
        pw, kw = self.to_device(w_loc, np.complex64)
        z, pz, kz = self._out(z, (self.R, self.K, self.T, self.F), np.complex64, 'any')
        route = C.c_int(0)
        self._chk(self.lib.disco_selftest_staged_step2(self.ctx, px, pm, pw, pz, int(bool(store_z)), C.addressof(route), self.stream))
        return z, self.STAGED_ROUTES[int(route.value)]

    def selftest_pending_matrices(self, P):
        """Rss, Rnn (R,Kl,F,P,P), NumPy, of the pending pencil, one left as tail blocks + kept step-1 blocks included (include/disco_hip.h).
        The library writes the pending pencil's own P x P (M or M + K - 1): the device arrays are sized for the larger whatever P says."""
        assert P in (self.M, self.M + self.K - 1), P
        n, nmax = self.R * self.Kl * self.F * P * P, self.R * self.Kl * self.F * (self.M + self.K - 1) ** 2
        Rss, Rnn = self.empty((nmax,), np.complex64), self.empty((nmax,), np.complex64)
        self._chk(self.lib.disco_selftest_pending_matrices(self.ctx, Rss.ptr, Rnn.ptr, self.stream))
        shape = (self.R, self.Kl, self.F, P, P)
        return Rss.numpy()[:n].reshape(shape), Rnn.numpy()[:n].reshape(shape)

    def reserve(self, own_workspace=1):
        """Allocate now what the whole-path calls would allocate on first use (0: partial-sum blocks only, 1: + the context's
        own workspace of tango_enhance / _iterated / _online, 2: + tango_reference's).  Afterwards a call is a fixed sequence of
        kernel launches on `self.stream` -- no allocation, no synchronisation -- and can be captured into a hipGraph."""
        self._chk(self.lib.disco_reserve(self.ctx, int(own_workspace)))

    def owned_bytes(self):
        """Device bytes the context owns (unchanged across a call <=> the call allocated nothing)."""
        return int(self.lib.disco_owned_bytes(self.ctx))

    def set_node_shard(self, first_node, node_count):
        """Hold only nodes [first_node, first_node + node_count) of every room (the rest live on other GPUs): the staged
        methods then take / return `node_count` nodes per room, while Zs / Zn / Z keep all K nodes (all-gathered z)."""
        self._chk(self.lib.disco_set_node_shard(self.ctx, first_node, node_count))
        self.k0, self.Kl = first_node, node_count

    def set_z_blocks(self, nodes_per_block):
        """The exchanged-signal arguments (Zs / Zn / Z) are laid out [K / nodes_per_block][R][nodes_per_block][T][F]: what an
        all-gather over ranks holding `nodes_per_block` nodes each delivers.  nodes_per_block = K: the plain [R][K][T][F]."""
        self._chk(self.lib.disco_set_z_blocks(self.ctx, nodes_per_block))
        self.zblk = nodes_per_block

    def set_lengths(self, lengths):
        """Per-room clip lengths (disco_set_lengths): `lengths` holds one valid length L_r <= length per room, or is None to restore
        the uniform batch.  The arrays keep their shapes; room r is processed as if run alone in an engine of length L_r: samples at
        and beyond L_r are never read, frames t >= T_r = 1 + L_r / hop are exact zeros in every spectrum and computed mask, output
        samples at and beyond L_r are exact zeros.  Masks passed in must be finite in the padding frames.  CRNN masks follow the lengths
        (dnn/inloop.py:tango_enhance_dnn, CRNN.predict_masks(..., frames=self.frames repeated per node)).  The online mode,
        `mask_ivad` and a node shard refuse while lengths are set."""
        if lengths is None:
            self._chk(self.lib.disco_set_lengths(self.ctx, None, 0))
            self._lengths = None
            return
        a = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int32)
        if not np.array_equal(a, np.asarray(lengths).reshape(-1)):
            raise ValueError('lengths must be integers')
        self._chk(self.lib.disco_set_lengths(self.ctx, a.ctypes.data, int(a.shape[0])))
        self._lengths = a.copy()

    @property
    def lengths(self):
        """(R,) int32: the valid length of every room (the engine's `length` for all of them while none are set)."""
        return np.full(self.R, self.Lsamp, np.int32) if self._lengths is None else self._lengths.copy()

    @property
    def frames(self):
        """(R,) int32: T_r = 1 + L_r / hop, the frames room r has (the rest of the T frames of the arrays are padding)."""
        return (1 + self.lengths // self.cfg.hop).astype(np.int32)

    def set_tuning(self, stft_frames_per_wave=0, cov_chunks=0, step2_chunks=0, istft_pairs=0):
        """Pin the launch geometry (0 = batch-size heuristic): lets a small batch run the code path of a large one."""
        self._chk(self.lib.disco_set_tuning(self.ctx, stft_frames_per_wave, cov_chunks, step2_chunks, istft_pairs))
        self._tuning = (int(stft_frames_per_wave), int(cov_chunks), int(step2_chunks), int(istft_pairs))

    OPTION_KEYS = ('room_cov', 'overlap_solves', 'solve_thread', 'solve_dpp', 'online_sq32', 'fuse_wide_istft', 'packed_x')

    def sibling(self, rooms, first_room=0):
        """A second engine for `rooms` rooms of the same problem: every field of the configuration (hop, reference microphone, mask
        settings, mu, padding, flags), the node shard and the layout of the exchanged signals are this engine's; options, tuning and
        stream follow with `follow(parent)`.  Per-room lengths: the sibling takes those of rooms [first_room, first_room + rooms)."""
        kid = Engine(rooms=rooms, nodes=self.K, lib=self.lib, **self._ctor)
        if (self.k0, self.Kl) != (0, self.K):
            kid.set_node_shard(self.k0, self.Kl)
        kid.follow(self, first_room)
        return kid

    def follow(self, parent, first_room=0):
        """Take over `parent`'s route options, pinned launch geometry, stream and (its slice of the) per-room lengths (idempotent; a
        few host calls)."""
        mine = None if parent._lengths is None else parent._lengths[first_room:first_room + self.R]
        if (mine is None) != (self._lengths is None) or (mine is not None and not np.array_equal(mine, self._lengths)):
            self.set_lengths(mine)
        for key in self.OPTION_KEYS:
            v = parent.get_option(key)
            if self.get_option(key) != v:
                self.set_option(key, v)
        if self._tuning != parent._tuning:
            self.set_tuning(*parent._tuning)
        self.stream = parent.stream

    def set_option(self, key, value):
        """Per-context switch between equivalent kernel routes (include/disco_hip.h: disco_set_option)."""
        self._chk(self.lib.disco_set_option(self.ctx, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        self._chk(self.lib.disco_get_option(self.ctx, key.encode(), C.byref(v)))
        return int(v.value)

    def stage_timing(self, enable=True):
        """Start (clearing) / stop the per-stage hipEvent timers of the whole-path calls."""
        self._chk(self.lib.disco_stage_timing(self.ctx, int(bool(enable))))

    def stage_report(self, max_stages=32):
        """-> {stage: (total_ms, launches, rooms)} for everything recorded since stage_timing(True); waits for the events.
        rooms = rooms processed summed over the launches (an overlapped call launches every stage once per half-batch)."""
        names = C.create_string_buffer(32 * max_stages)
        ms = (C.c_float * max_stages)()
        cnt = (C.c_int * max_stages)()
        rooms = (C.c_int64 * max_stages)()
        n = self.lib.disco_stage_report(self.ctx, names, ms, cnt, rooms, max_stages)
        if n < 0:
            self._chk(n)
        return {names.raw[32 * i:32 * i + 32].split(b'\0', 1)[0].decode(): (float(ms[i]), int(cnt[i]), int(rooms[i])) for i in range(n)}

    def sync(self):
        self._chk(self.lib.disco_sync(self.ctx, self.stream))

    def to_device(self, a, dtype):
        """-> (device pointer, keep-alive object)."""
        if a is None:
            return None, None
        if isinstance(a, DevBuf):
            assert a.dtype == np.dtype(dtype), (a.dtype, dtype)
            return a.ptr, a
        if hasattr(a, 'data_ptr'):                       # torch tensor: zero-copy, so it must already BE what the kernel reads
            want = np.dtype(dtype)
            tname = str(a.dtype).replace('torch.', '')
            ok = {'float32': ('float32',), 'float64': ('float64',), 'uint8': ('uint8',),
                  'complex64': ('complex64', 'float32')}.get(want.name, (want.name,))     # complex64 also as its (..., 2) float32 view
            if tname not in ok:
                raise TypeError(f'expected a {want.name} tensor, got torch.{tname} (the kernels would reinterpret the bytes)')
            if not a.is_contiguous():
                raise ValueError('device tensors must be contiguous')
            dev = a.device
            if dev.type == 'cuda' and dev.index is not None and dev.index != self.cfg.device and not self._host_pointers_ok:
                raise ValueError(f'tensor lives on cuda:{dev.index}, this engine on device {self.cfg.device}')
            if dev.type != 'cuda' and not self._host_pointers_ok:
                raise ValueError('torch tensors must live on the GPU (pass a numpy array for a host->device copy)')
            return a.data_ptr(), a
        a = np.ascontiguousarray(a, dtype=dtype)
        b = DevBuf(self, a.shape, dtype)
        self._chk(self.lib.disco_h2d(self.ctx, b.ptr, a.ctypes.data, b.nbytes, self.stream))
        self.sync()
        return b.ptr, b

    def empty(self, shape, dtype):
        return DevBuf(self, shape, dtype)

    # ---- stage kernels (names follow include/disco_hip.h)
    def stft(self, x, out=None):
        """x (n_sig, chans, L) float32 -> X (n_sig, T, F, chans) complex64   [lb.core.stft, tango.py:335]
        out: optional caller-owned device array (DevBuf or torch complex64 tensor) of n_sig * T * F * chans elements."""
        n_sig, chans, Ls = x.shape
        assert Ls == self.Lsamp
        px, kx = self.to_device(x, np.float32)
        out, po, ko = self._out(out, (n_sig, self.T, self.F, chans), np.complex64, 'any')
        self._chk(self.lib.disco_stft(self.ctx, px, n_sig, chans, po, self.stream))
        return out

    def istft(self, Z, out=None):
        """Z (n_sig, T, F) complex64 -> (n_sig, L) float32   [lb.core.istft, tango.py:528]
        out: optional caller-owned device array (DevBuf or torch tensor) of n_sig * L float32 to write into."""
        n_sig = Z.shape[0]
        assert tuple(Z.shape[1:]) == (self.T, self.F)
        pz, kz = self.to_device(Z, np.complex64)
        out, po, ko = self._out(out, (n_sig, self.Lsamp), np.float32, 'size')
        self._chk(self.lib.disco_istft(self.ctx, pz, n_sig, po, self.stream))
        return out

    def tf_mask(self, S, N, type='irm1', bin_thr=0.0):
        mt, mp = parse_mask_type(type)
        assert tuple(S.shape) == tuple(N.shape)
        ps, ks = self.to_device(S, np.complex64)
        pn, kn = self.to_device(N, np.complex64)
        m = self.empty(S.shape, np.float32)
        self._chk(self.lib.disco_tf_mask(self.ctx, ps, pn, int(np.prod(S.shape)), mt, mp, bin_thr, m.ptr, self.stream))
        return m

    def mask_oracle(self, s_ref, n_ref):
        """s_ref, n_ref (n_sig, L) -> mask (n_sig, T, F)   [get_mask at the reference mic, tango.py:338-342]"""
        n_sig = s_ref.shape[0]
        ps, ks = self.to_device(s_ref, np.float32)
        pn, kn = self.to_device(n_ref, np.float32)
        m = self.empty((n_sig, self.T, self.F), np.float32)
        self._chk(self.lib.disco_mask_oracle(self.ctx, ps, pn, n_sig, m.ptr, self.stream))
        return m

    def source_masks(self, images, want_mix=True):
        """images (S, n_sig, L), source-major -> (masks (S, n_sig, T, F), mix (n_sig, T, F) complex64 or None): the mask of every
        talker's image against the sum of the others and the spectrum of the sum of all, in one transform pass (disco_source_masks;
        get_masks, gen_meetit/convolve_signals.py:166-188).  The mask kind is the engine's.  2 <= S <= 8."""
        S, n_sig, Ls = (int(v) for v in images.shape)
        assert Ls == self.Lsamp
        pi, ki = self.to_device(images, np.float32)
        m = self.empty((S, n_sig, self.T, self.F), np.float32)
        mix = self.empty((n_sig, self.T, self.F), np.complex64) if want_mix else None
        self._chk(self.lib.disco_source_masks(self.ctx, pi, S, n_sig, m.ptr, _ptr(mix), self.stream))
        return m, mix

    def cov_masked(self, X, mask, Zs=None, Zn=None, mask_remote=True, Rss_out=True):
        """X (R,K,T,F,M), mask (R,K,T,F)[, Zs, Zn (R,K,T,F)] -> Rss, Rnn (R,K,F,P,P)   [tango.py:357-364, 433-440]"""
        P = self.M + (self.K - 1 if Zs is not None else 0)
        px, kx = self.to_device(X, np.complex64)
        pm, km = self.to_device(mask, np.float32)
        pzs, kzs = self.to_device(Zs, np.complex64)
        pzn, kzn = self._alias(Zn, Zs, (pzs, kzs), np.complex64, none='null')
        # Rss_out=False: leave the partial sums in the context for gevd_mwf_r1_pending
        Rss = self.empty((self.R, self.Kl, self.F, P, P), np.complex64) if Rss_out else None
        Rnn = self.empty((self.R, self.Kl, self.F, P, P), np.complex64) if Rss_out else None
        self._chk(self.lib.disco_cov_masked(self.ctx, px, pm, pzs, pzn, int(bool(mask_remote)), P, _ptr(Rss), _ptr(Rnn), self.stream))
        return Rss, Rnn

    def gevd_mwf_r1(self, Rss, Rnn, mu=None, want_t1=True):
        """Rss, Rnn (..., P, P) -> w, t1 (..., P)   [intern_filter(..., 'gevd', rank=1), internal_formulas.py:56-73]"""
        shape, P, n_prob, pa, pb, keep = self._pencils(Rss, Rnn)
        w = self.empty(shape[:-1], np.complex64)
        t1 = self.empty(shape[:-1], np.complex64) if want_t1 else None
        self._chk(self.lib.disco_gevd_mwf_r1(self.ctx, pa, pb, n_prob, P, self.cfg.mu if mu is None else mu, w.ptr, _ptr(t1), self.stream))
        return w, t1

    def gevd_mwf(self, Rxx, Rnn, rank, mu=None, want_t1=True):
        """Rxx, Rnn (..., P, P) -> w, t1 (..., P)   [intern_filter(..., 'gevd', rank), internal_formulas.py:56-73, for a kept rank >= 0;
        rank >= P is full rank]"""
        shape, P, n_prob, pa, pb, keep = self._pencils(Rxx, Rnn)
        w = self.empty(shape[:-1], np.complex64)
        t1 = self.empty(shape[:-1], np.complex64) if want_t1 else None
        self._chk(self.lib.disco_gevd_mwf(self.ctx, pa, pb, n_prob, P, int(rank), self.cfg.mu if mu is None else mu, w.ptr, _ptr(t1),
                                          self.stream))
        return w, t1

    def mwf_filter(self, Rxx, Rnn, type='r1-mwf', mu=None):
        """intern_filter's 'r1-mwf' / 'mwf' branches (internal_formulas.py:45-54, 74-76), batched: (..., P, P) -> w (..., P)."""
        shape, P, n_prob, pa, pb, keep = self._pencils(Rxx, Rnn)
        w = self.empty(shape[:-1], np.complex64)
        self._chk(self.lib.disco_mwf_filter(self.ctx, pa, pb, n_prob, P, self.cfg.mu if mu is None else mu,
                                            {'r1-mwf': 1, 'mwf': 2}[type], w.ptr, self.stream))
        return w

    def gevd_mwf_r1_pending(self, P, mu=None, want_t1=False, out=None):
        """Solve straight from the partial sums the last covariance call left in the context.
        out: optional caller-owned (R, Kl, F, P) complex64 device array (DevBuf or torch tensor) for the filters."""
        w, pw, kw = self._out(out, (self.R, self.Kl, self.F, P), np.complex64, 'shape')
        t1 = self.empty((self.R, self.Kl, self.F, P), np.complex64) if want_t1 else None
        self._chk(self.lib.disco_gevd_mwf_r1_pending(self.ctx, self.cfg.mu if mu is None else mu, pw, _ptr(t1), self.stream))
        return w, t1

    def apply(self, X, w, Z=None, conj=True, out=None):
        """out = w^H [X ; Z_-k] (conj=True) or w^T [...]   [tango.py:369-374, 445-450]
        out: optional caller-owned (R, Kl, T, F) complex64 device array (DevBuf or torch tensor) to write into."""
        P = self.M + (self.K - 1 if Z is not None else 0)
        px, kx = self.to_device(X, np.complex64)
        pz, kz = self.to_device(Z, np.complex64)
        pw, kw = self.to_device(w, np.complex64)
        out, po, ko = self._out(out, (self.R, self.Kl, self.T, self.F), np.complex64, 'shape')
        self._chk(self.lib.disco_apply(self.ctx, px, pz, pw, P, int(bool(conj)), po, self.stream))
        return out

    def apply_istft(self, X, w, Z, out=None, yf_out=None):
        """iSTFT(w^H [X ; Z_-k]) in ONE pass (disco_apply_istft_fused: `apply` followed by `istft` with the filtered spectra kept on chip)
        -> (R, Kl, L) float32, or None when the kernel is not built for this (mics, nodes) shape (the caller then runs the two calls).
        yf_out: optional caller-owned (R, Kl, T, F) complex64 device array that also receives the filtered spectra."""
        px, kx = self.to_device(X, np.complex64)
        pz, kz = self.to_device(Z, np.complex64)
        pw, kw = self.to_device(w, np.complex64)
        out, po, ko = self._out(out, (self.R, self.Kl, self.Lsamp), np.float32, 'size')
        pyf, kyf = self.to_device(yf_out, np.complex64)              # unchecked; None: the spectra are not stored
        rc = self.lib.disco_apply_istft_fused(self.ctx, px, pz, pw, pyf, po, self.stream)
        if rc == -2:                                              # DISCO_E_UNSUPPORTED: shape not built
            return None
        self._chk(rc)
        return out

    def filter_head(self, w_glo, out=None):
        """w_glo (R, Kl, F, P) -> its local part (R, Kl, F, M): the re-compression filter of the iterated scheme.
        out: optional caller-owned device array for it."""
        P = int(w_glo.shape[-1])
        pw, kw = self.to_device(w_glo, np.complex64)
        w_loc, po, ko = self._out(out, (self.R, self.Kl, self.F, self.M), np.complex64, 'shape')
        self._chk(self.lib.disco_filter_head(self.ctx, pw, P, po, self.stream))
        return w_loc

    def noise_residual(self, X, z):
        px, kx = self.to_device(X, np.complex64)
        pz, kz = self.to_device(z, np.complex64)
        zn = self.empty((self.R, self.Kl, self.T, self.F), np.complex64)
        self._chk(self.lib.disco_noise_residual(self.ctx, px, pz, zn.ptr, self.stream))
        return zn

    def stft_cov_fused(self, y, mask_z, X_out=None, want_cov=True):
        """y (R,Kl,M,L), mask_z (R,Kl,T,F) -> X (R,Kl,T,F,M), Rss, Rnn (R,Kl,F,M,M) in one pass over the samples (Kl = K unless a node
        shard is active).  want_cov=False: the covariances stay in the context as partial sums for gevd_mwf_r1_pending (Rss = Rnn = None).
        X_out: caller-owned device array for the spectra."""
        py, ky = self.to_device(y, np.float32)
        pm, km = self.to_device(mask_z, np.float32)
        Kl = self.Kl
        X, px, kx = self._out(X_out, (self.R, Kl, self.T, self.F, self.M), np.complex64, 'any')
        Rss = self.empty((self.R, Kl, self.F, self.M, self.M), np.complex64) if want_cov else None
        Rnn = self.empty((self.R, Kl, self.F, self.M, self.M), np.complex64) if want_cov else None
        self._chk(self.lib.disco_stft_cov_fused(self.ctx, py, pm, px, _ptr(Rss), _ptr(Rnn), self.stream))
        return X, Rss, Rnn

    def step2_cov_fused(self, X, mask_w, w_loc, want_z=True):
        """Fused apply-1 + in-register z exchange + step-2 covariance -> Rss, Rnn (R,K,F,P,P)[, z (R,K,T,F)]."""
        P = self.M + self.K - 1
        px, kx = self.to_device(X, np.complex64)
        pm, km = self.to_device(mask_w, np.float32)
        pw, kw = self.to_device(w_loc, np.complex64)
        z = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_z else None
        Rss = self.empty((self.R, self.K, self.F, P, P), np.complex64)
        Rnn = self.empty((self.R, self.K, self.F, P, P), np.complex64)
        self._chk(self.lib.disco_step2_cov_fused(self.ctx, px, pm, pw, _ptr(z), Rss.ptr, Rnn.ptr, self.stream))
        return Rss, Rnn, z

    def step2_cov_fused_reuse(self, X, mask_w, w_loc, want_z=False):
        """step2_cov_fused when mask_w is the step-1 mask and the step-1 partial sums of `stft_cov_fused` are still in the
        context: their M x M block is not recomputed.  Leaves the pencil pending for `gevd_mwf_r1_pending(M+K-1)`."""
        px, kx = self.to_device(X, np.complex64)
        pm, km = self.to_device(mask_w, np.float32)
        pw, kw = self.to_device(w_loc, np.complex64)
        z = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_z else None
        self._chk(self.lib.disco_step2_cov_fused_reuse(self.ctx, px, pm, pw, _ptr(z), self.stream))
        return z

    def step2_apply_fused(self, X, w_loc, w_glo, want_z=False):
        px, kx = self.to_device(X, np.complex64)
        pl, kl = self.to_device(w_loc, np.complex64)
        pg, kg = self.to_device(w_glo, np.complex64)
        z = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_z else None
        yf = self.empty((self.R, self.K, self.T, self.F), np.complex64)
        self._chk(self.lib.disco_step2_apply_fused(self.ctx, px, pl, pg, _ptr(z), yf.ptr, self.stream))
        return yf, z

    def step2_apply_istft_fused(self, X, w_loc, w_glo):
        """X, w_loc, w_glo -> enhanced time signals (R, K, L); yf stays on chip."""
        px, kx = self.to_device(X, np.complex64)
        pl, kl = self.to_device(w_loc, np.complex64)
        pg, kg = self.to_device(w_glo, np.complex64)
        out = self.empty((self.R, self.K, self.Lsamp), np.float32)
        self._chk(self.lib.disco_step2_apply_istft_fused(self.ctx, px, pl, pg, out.ptr, self.stream))
        return out

    def tango_enhance_iterated(self, y, mask_z, mask_w=None, iters=2):
        """DANSE-style continuation of the two-step scheme (BASELINE.json configs[4]; not in the reference): step 2 is
        run `iters` times, each time with z_k <- w_glo,k[:M]^H y_k.  iters=1 is exactly offline_tango's y branch.
        Staged kernels (z materialised), one C call (disco_tango_enhance_iterated).  Returns (out (R,K,L), yf (R,K,T,F))."""
        py, ky = self.to_device(y, np.float32)
        pmz, kmz = self.to_device(mask_z, np.float32)
        pmw, kmw = self._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='same')
        out = self.empty((self.R, self.K, self.Lsamp), np.float32)
        yf = self.empty((self.R, self.K, self.T, self.F), np.complex64)
        self._chk(self.lib.disco_tango_enhance_iterated(self.ctx, py, pmz, pmw, iters, out.ptr, None, yf.ptr, None, 0, self.stream))
        return out, yf

    def tango_reference(self, y, s, n, mask_z=None, mask_w=None, mask_for_z='local', steps=3, want=None):
        """offline_tango's nine outputs in ONE device-resident call (disco_tango_reference): y, s, n (R,K,M,L) float32;
        mask_z / mask_w (R,K,T,F) float32 or None (oracle TF masks of the engine's mask type); steps 1 | 2 | 3.
        Returns {name: DevBuf (R,K,T,F)} for the names in `want` (default: all that the requested steps produce)."""
        step1 = ('z_y', 'z_s', 'z_n', 'zn', 'masks_z')
        step2 = ('yf', 'sf', 'nf', 'mask_w')
        names = [nm for nm in (step1 if steps & 1 else ()) + (step2 if steps & 2 else ())]
        if want is not None:
            names = [nm for nm in names if nm in want]
        py, ky = self.to_device(y, np.float32)
        ps, ks = self.to_device(s, np.float32)
        pn, kn = self.to_device(n, np.float32)
        pmz, kmz = self.to_device(mask_z, np.float32)
        pmw, kmw = self._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='null')         # None is the oracle mask, not mask_z
        bufs = {nm: self.empty((self.R, self.K, self.T, self.F), np.float32 if nm.startswith('mask') else np.complex64) for nm in names}
        outs = L.DiscoRefOutputs(**{nm: b.ptr for nm, b in bufs.items()})
        self._chk(self.lib.disco_tango_reference(self.ctx, py, ps, pn, pmz, pmw, L.MASK_FOR_Z[mask_for_z], steps, C.byref(outs), None, 0,
                                                 self.stream))
        return bufs

    # ---- whole path
    def workspace_bytes(self):
        return int(self.lib.disco_workspace_bytes(self.ctx))

    def tango_enhance(self, y, mask_z, mask_w=None, want_z=True, want_yf=True, out=None, workspace=None):
        """y (R,K,M,L), masks (R,K,T,F) -> out (R,K,L) [, z_y, yf (R,K,T,F)]: offline_tango's y branch + iSTFT."""
        py, ky = self.to_device(y, np.float32)
        pmz, kmz = self.to_device(mask_z, np.float32)
        pmw, kmw = self._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='same')
        out, po, ko = self._out(out, (self.R, self.K, self.Lsamp), np.float32, 'any')
        z = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_z else None
        yf = self.empty((self.R, self.K, self.T, self.F), np.complex64) if want_yf else None
        pws, kws = self.to_device(workspace, np.uint8)
        wsb = 0 if workspace is None else (workspace.nbytes if hasattr(workspace, 'nbytes') else workspace.numel())
        self._chk(self.lib.disco_tango_enhance(self.ctx, py, pmz, pmw, po, _ptr(z), _ptr(yf), pws, wsb, self.stream))
        return out, z, yf


class _OnlineStream:
    def __init__(self, eng, lambda_cor, update_every, init_diag):
        self.eng, self.par = eng, (float(lambda_cor), int(update_every), float(init_diag))
        self.hops = 0
        self.state = eng.empty((int(eng.lib.disco_online_state_bytes(eng.ctx)),), np.uint8)
        self.ws = None

    def frames_of(self, n_hops, last=False):
        return n_hops + (1 if last else 0)

    def push(self, y_new, mask_z, mask_w=None, last=False):
        """The next n_hops >= 1 hops of every channel (the first push: >= 2) -> the samples that became final.  last=True also completes the
        frame centred at the end of the signal; it needs new samples in the same call (the stream cannot be flushed empty-handed: the
        caller marks its last chunk)."""
        e = self.eng
        R, K, M, n = y_new.shape
        H = (e.F - 1)                                        # hop = n_fft / 2 = F - 1
        assert (R, K, M) == (e.R, e.K, e.M) and n % H == 0 and n > 0
        n_hops = n // H
        n_new = n_hops + (1 if last else 0)
        n_out = H * (n_new - (1 if self.hops == 0 else 0))
        # the C entry point receives bare pointers and reads n_new mask rows per (room, node): a mask that is one frame short (the extra
        # frame of the LAST chunk forgotten) would be an out-of-bounds device read -- checked here
        for nm, mk in (('mask_z', mask_z), ('mask_w', mask_w)):
            if mk is not None and hasattr(mk, 'shape'):
                assert tuple(mk.shape) == (R, K, n_new, e.F), f'{nm}: expected {(R, K, n_new, e.F)} (n_hops + 1 frames with last=True), got {tuple(mk.shape)}'
        py, ky = e.to_device(np.ascontiguousarray(y_new) if isinstance(y_new, np.ndarray) else y_new, np.float32)
        pmz, kmz = e.to_device(mask_z, np.float32)
        pmw, kmw = e._alias(mask_w, mask_z, (pmz, kmz), np.float32, none='same')
        need = int(e.lib.disco_online_stream_workspace_bytes(e.ctx, n_hops))
        if self.ws is None or self.ws.nbytes < need:
            self.ws = e.empty((need,), np.uint8)
        out = e.empty((R, K, max(n_out, 1)), np.float32)
        lam, ue, idg = self.par
        e._chk(e.lib.disco_tango_online_stream(e.ctx, py, n_hops, pmz, pmw, lam, ue, idg, self.hops, int(bool(last)), self.state.ptr, out.ptr,
                                               self.ws.ptr, self.ws.nbytes, e.stream))
        self.hops += n_hops
        res = out.numpy()[:, :, :n_out]
        return res
