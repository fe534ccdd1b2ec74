"""Call trace of disco_amd/engine.py against a recording stand-in for libdisco_hip.so (CPU only, no library, no emulator).

`Engine(lib=...)` takes any object.  `RecordingLib` answers every `disco_*` entry point by appending (name, arguments) to a list and
returning 0; allocations get increasing fake addresses, so that every pointer a call receives can be named (allocation number, byte offset).
`run_script` drives every public method of `Engine` and `_OnlineStream.push` through the stand-in, each in every dialect it has (NumPy /
DevBuf / CPU-torch inputs, optional outputs, `out=`, aliased arguments, the three forms of `stop`, chunk walks, argument errors).

    python tools/engine_call_trace.py PARENT_TREE CHANGE_TREE [--out profiles/engine_call_trace.txt]     compare two source trees
    python tools/engine_call_trace.py PARENT_TREE CHANGE_TREE --time                                     host overhead of one call
    python tools/engine_call_trace.py --dump TREE                                                        one tree's trace as JSON

Two trees agree when their normalised traces are identical call for call apart from the positions of the `disco_dev_free` calls (when
Python drops a buffer is not part of the contract; that no call receives a pointer into a freed allocation is, and is asserted), and when
the exceptions the script provokes are identical in type and message.  Methods that only one of the two trees has (a change that adds one)
are scripted in a marked section at the end, which is then left out of the comparison: everything before it lines up allocation for allocation.
"""
import argparse
import bisect
import ctypes as C
import gc
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

T_FRAMES, N_FREQ = 9, 9                 # what disco_n_frames / disco_n_freq answer: length 64, n_fft 16, hop 8
DEV_BASE = 1 << 52                      # fake device addresses start here (beyond any host address)
CTX_BASE = 0xC7C70000


class RecordingLib:
    """A plain object with the attributes of the bound library.  trace: [name, [normalised arguments]] per call."""

    def __init__(self, prototypes):
        self.proto = prototypes
        self.trace = []
        self.starts, self.sizes, self.live = [], [], set()
        self.last_use = {}              # allocation number -> index of the last call that received a pointer into it
        self.frees = []                 # (allocation number, index of its disco_dev_free, last use or None)
        self.violations = []            # pointers into freed allocations, double frees
        self.tensors = []               # (data_ptr, bytes, the tensor: kept, so that no host array takes its place) of the script's torch tensors
        self.ctxs = {}
        self.options = {}
        self.per_item = 1000            # bytes per item the *_workspace_bytes of the chunked metrics answer (0: unsupported shape)
        self.returns = {}               # name -> return code, for the error paths

    def note_tensor(self, t):
        self.tensors.append((t.data_ptr(), t.numel() * t.element_size(), t))
        return t

    def __getattr__(self, name):
        if not name.startswith('disco_'):
            raise AttributeError(name)
        types = self.proto[name][1]

        def call(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            idx = len(self.trace)
            entry = [name, [self._norm(a, t, idx, i == 0, name != 'disco_dev_free') for i, (a, t) in enumerate(zip(args, types))]]
            self.trace.append(entry)
            return getattr(self, '_' + name[6:], self._plain)(name, args, entry)
        self.__dict__[name] = call
        return call

    # ---- normalisation: device address -> (allocation, offset), torch data_ptr -> (tensor, offset), host address -> 'host'
    def _alloc_of(self, p):
        k = bisect.bisect_right(self.starts, p) - 1
        assert k >= 0 and p - self.starts[k] <= self.sizes[k], hex(p)
        return k

    def _pointer(self, p, idx, first, use):
        if p is None:
            return None
        p = int(p)
        if first and p in self.ctxs:
            return ['ctx', self.ctxs[p]]
        if p >= DEV_BASE:
            k = self._alloc_of(p)
            if use:
                if k not in self.live:
                    self.violations.append(f'call {idx} receives a pointer into allocation {k}, which is freed')
                self.last_use[k] = idx
            return ['dev', k, p - self.starts[k]]
        for k, (base, nbytes, _) in enumerate(self.tensors):
            if base <= p < base + max(nbytes, 1):
                return ['tensor', k, p - base]
        return 'host'

    def _norm(self, a, t, idx, first, use):
        if t is C.c_void_p:
            return self._pointer(a, idx, first, use)
        if t is C.c_char_p:
            return type(a).__name__ if isinstance(a, C.Array) else a.decode()
        if isinstance(t, type) and issubclass(t, C._Pointer):
            obj = getattr(a, '_obj', a)                              # byref(x) -> x
            if isinstance(obj, C.Structure):
                return {nm: (self._pointer(getattr(obj, nm), idx, False, use) if ft is C.c_void_p else
                             list(getattr(obj, nm)) if isinstance(getattr(obj, nm), C.Array) else getattr(obj, nm)) for nm, ft in obj._fields_}
            return type(obj).__name__ if isinstance(obj, C.Array) else ['ref', obj.value]
        return float(a) if t is C.c_float else int(a)

    # ---- the entry points that answer something
    def _plain(self, name, args, entry):
        return self.returns.get(name, 0)

    def _version(self, name, args, entry):
        return b'recording stand-in (no device code)'

    def _last_error(self, name, args, entry):
        return b''

    def _create(self, name, args, entry):
        v = CTX_BASE + 16 * len(self.ctxs)
        self.ctxs[v] = len(self.ctxs)
        args[0]._obj.value = v
        return self.returns.get(name, 0)

    def _dev_alloc(self, name, args, entry):
        nbytes = int(args[1])
        addr = self.starts[-1] + (self.sizes[-1] + 511) // 256 * 256 if self.starts else DEV_BASE
        self.live.add(len(self.starts))
        entry.append(['alloc', len(self.starts)])
        self.starts.append(addr)
        self.sizes.append(nbytes)
        args[2]._obj.value = addr
        return 0

    def _dev_free(self, name, args, entry):
        k = self._alloc_of(int(args[1]))
        if k not in self.live:
            self.violations.append(f'allocation {k} is freed twice')
        self.live.discard(k)
        self.frees.append((k, len(self.trace) - 1, self.last_use.get(k)))
        return 0

    def _h2d(self, name, args, entry):
        entry.append(['crc32', zlib.crc32(C.string_at(args[2], args[3]))])       # what was uploaded, not only where to
        return 0

    def _d2h(self, name, args, entry):
        C.memset(args[1], 0, args[3])
        return 0

    def _n_frames(self, name, args, entry):
        return T_FRAMES

    def _n_freq(self, name, args, entry):
        return N_FREQ

    def _set_option(self, name, args, entry):
        self.options[args[0], args[1]] = int(args[2])
        return 0

    def _get_option(self, name, args, entry):
        args[2]._obj.value = self.options.get((args[0], args[1]), 0)
        return 0

    def _selftest_staged_step2(self, name, args, entry):
        C.c_int.from_address(args[6]).value = 1
        return 0

    def _bss_workspace_bytes(self, name, args, entry):
        return self.per_item * int(args[1])

    _stoi_workspace_bytes = _estoi_workspace_bytes = _bss_workspace_bytes

    def _lag_corr_workspace_bytes(self, name, args, entry):
        return 64

    def _workspace_bytes(self, name, args, entry):
        return 4096

    _reference_workspace_bytes = _owned_bytes = _workspace_bytes

    def _online_state_bytes(self, name, args, entry):
        return 256

    def _online_stream_workspace_bytes(self, name, args, entry):
        return 128 * int(args[1])


def load_engine(tree):
    """disco_amd.engine and disco_amd._lib of the source tree `tree`."""
    sys.path.insert(0, os.path.abspath(tree))
    from disco_amd import _lib, engine
    assert os.path.abspath(engine.__file__).startswith(os.path.abspath(tree) + os.sep), engine.__file__
    return engine, _lib


R, K, M, LS = 2, 2, 2, 64
KINDS = ('np', 'dev', 'torch')


def run_script(engine, lib):
    """The fixed script.  -> (exceptions [(step, type, message)], sorted names of the methods called)."""
    import torch
    Engine = engine.Engine
    eng = Engine(rooms=R, nodes=K, mics=M, length=LS, n_fft=16, lib=lib)
    T, F = eng.T, eng.F
    errors, covered, counter, absent = [], set(), [0], set()

    def mk(kind, shape, dtype=np.float32, fill=None):
        counter[0] += 1
        a = (np.arange(int(np.prod(shape))) % 7 + counter[0]).astype(dtype).reshape(shape) if fill is None else np.full(shape, fill, dtype)
        if kind == 'dev':
            return eng.to_device(a, dtype)[1]
        return lib.note_tensor(torch.from_numpy(a)) if kind == 'torch' else a

    def describe(v, given, pointers=False):
        """What a method returned, for the trace: the caller's own object, a DevBuf by allocation, an array by shape and type."""
        if v is not None and any(v is g for g in given):
            return 'an argument of the call'
        if pointers and isinstance(v, int):
            return lib._pointer(v, -1, False, False)
        if isinstance(v, engine.DevBuf):
            return ['DevBuf', lib._pointer(v.ptr, -1, False, False), list(v.shape), str(v.dtype)]
        if isinstance(v, np.ndarray):
            return ['ndarray', list(v.shape), str(v.dtype)]
        if isinstance(v, (tuple, list)):
            return [describe(x, given, pointers) for x in v]
        if isinstance(v, dict):
            return {k: describe(x, given) for k, x in v.items()}
        return v if isinstance(v, (int, float, str, type(None))) else type(v).__name__

    def call(name, *a, _on=None, **kw):
        """One step: the method's name goes into the trace, so that the two traces line up; what it raises is recorded, not raised."""
        on = eng if _on is None else _on
        if not hasattr(on, name):                                       # a method this tree does not have (yet): nothing is recorded, and the
            absent.add(name)                                            # comparison leaves the other tree's steps of that name out
            return None
        covered.add(('push' if name == 'push' else name))
        lib.trace.append(['step', name])
        try:
            attr = getattr(on, name)
            res = attr(*a, **kw) if callable(attr) else attr            # `lengths` and `frames` are properties
            lib.trace.append(['returned', describe(res, list(a) + list(kw.values()), name == 'to_device')])
            return res
        except Exception as e:
            errors.append((len(lib.trace), name, type(e).__name__, str(e)))
            lib.trace.append(['raised', type(e).__name__, str(e)])
            return None

    c64, f32 = np.complex64, np.float32
    for kind in KINDS:
        mkc = lambda *shape: mk(kind, shape, c64)
        mkf = lambda *shape: mk(kind, shape, f32)
        y, mz, mw = mkf(R, K, M, LS), mkf(R, K, T, F), mkf(R, K, T, F)
        X, Z, Zn = mkc(R, K, T, F, M), mkc(R, K, T, F), mkc(R, K, T, F)
        w_loc, w_glo = mkc(R, K, F, M), mkc(R, K, F, M + K - 1)
        # the whole-path calls: mask_w None / the same object / another object; optional outputs; out= of each kind
        for mask_w in (None, mz, mw):
            call('tango_enhance', y, mz, mask_w)
            call('tango_online', y, mz, mask_w, update_every=2)
            call('tango_enhance_iterated', y, mz, mask_w, iters=3)
        for okind in KINDS:
            call('tango_enhance', y, mz, want_z=False, out=mk(okind, (R, K, LS)))
            call('tango_online', y, mz, want_yf=False, out=mk(okind, (R, K, LS)))
            call('stft', mkf(3, 2, LS), out=mk(okind, (3, T, F, 2), c64))
            call('stft_cov_fused', y, mz, X_out=mk(okind, (R, K, T, F, M), c64))
            call('selftest_staged_step2', X, mz, w_loc, z=mk(okind, (R, K, T, F), c64))
            call('apply_istft', X, w_glo, Z, yf_out=mk(okind, (R, K, T, F), c64))
            # the checked outputs: a NumPy array is refused
            call('istft', Z.reshape(R * K, T, F), out=mk(okind, (R * K * LS,)))
            call('bss_estimates', mkf(3, LS), mkf(3, LS), mkf(3, LS), out=mk(okind, (3 * 6, LS)))
            call('apply_istft', X, w_glo, Z, out=mk(okind, (R * K, LS)))
            call('gevd_mwf_r1_pending', M, out=mk(okind, (R, K, F, M), c64))
            call('apply', X, w_loc, out=mk(okind, (R, K, T, F), c64))
            call('filter_head', w_glo, out=mk(okind, (R, K, F, M), c64))
        call('tango_enhance', y, mz, want_z=False, want_yf=False, workspace=mk('dev', (4096,), np.uint8))
        call('tango_enhance', y, mz, workspace=mk('torch', (4096,), np.uint8))
        call('workspace_bytes')
        for m_z, m_w in ((None, None), (mz, None), (mz, mz), (mz, mw), (None, mw)):
            call('tango_reference', y, mkf(R, K, M, LS), mkf(R, K, M, LS), mask_z=m_z, mask_w=m_w)
        call('tango_reference', y, y, y, steps=1, want=('z_y', 'masks_z'), mask_for_z='distant')
        call('tango_reference', y, y, y, steps=2)
        # the online mode
        call('online_mwf', X, mz)
        call('online_mwf', X, mz, Z=Z, lambda_cor=0.9, mu=2.0, update_every=4, want_w=True)
        st = call('online_stream', 0.9, 2, 1e-2)
        H = F - 1
        call('push', mkf(R, K, M, 2 * H), mkf(R, K, 2, F), _on=st)
        m2 = mkf(R, K, 1, F)
        call('push', mkf(R, K, M, H), m2, m2, _on=st)
        call('push', mkf(R, K, M, 3 * H), mkf(R, K, 4, F), mkf(R, K, 4, F), last=True, _on=st)
        call('push', mkf(R, K, M, H), mkf(R, K, 1, F), last=True, _on=st)                  # the mask one frame short
        call('frames_of', 3, True, _on=st)
        del st
        # stage kernels
        call('stft', mkf(3, 2, LS))
        call('stft', mkf(3, 2, LS - 1))
        call('istft', Z.reshape(R * K, T, F))
        call('istft', Z.reshape(R * K, T, F), out=mk('dev', (R * K, LS + 1)))
        call('tf_mask', Z, Zn)
        call('tf_mask', Z, Zn, type='ibm2', bin_thr=3.0)
        call('tf_mask', Z, Zn, type='xyz1')
        call('mask_oracle', mkf(R * K, LS), mkf(R * K, LS))
        call('mask_ivad', mkf(R * K, LS))
        call('cov_masked', X, mz)
        call('cov_masked', X, mz, Zs=Z, Zn=Z)
        call('cov_masked', X, mz, Zs=Z, Zn=Zn, mask_remote=False)
        call('cov_masked', X, mz, Zs=Z)
        call('cov_masked', X, mz, Rss_out=False)
        Rss, Rnn = mkc(R, K, F, M, M), mkc(R, K, F, M, M)
        call('gevd_mwf_r1', Rss, Rnn)
        call('gevd_mwf_r1', Rss, Rnn, mu=0.5, want_t1=False)
        call('gevd_mwf', Rss, Rnn, 2)
        call('gevd_mwf', Rss, Rnn, 1, mu=0.5, want_t1=False)
        call('mwf_filter', Rss, Rnn)
        call('mwf_filter', Rss, Rnn, type='mwf', mu=0.5)
        call('gevd_mwf_r1_pending', M)
        call('gevd_mwf_r1_pending', M + K - 1, mu=0.5, want_t1=True)
        call('gevd_mwf_r1_pending', M, out=mk('dev', (R, K, F, M + 1), c64))
        call('apply', X, w_loc)
        call('apply', X, w_glo, Z=Z, conj=False)
        call('apply', X, w_loc, out=mk('dev', (R, K, T * F), c64))
        call('apply_istft', X, w_glo, Z)
        call('apply_istft', X, w_glo, Z, out=mk('dev', (R * K, LS - 1)))
        lib.returns['disco_apply_istft_fused'] = -2
        call('apply_istft', X, w_glo, Z)
        lib.returns['disco_apply_istft_fused'] = -1
        call('apply_istft', X, w_glo, Z)
        del lib.returns['disco_apply_istft_fused']
        call('filter_head', w_glo)
        call('filter_head', w_glo, out=mk('dev', (R, K, F, M + 1), c64))
        call('noise_residual', X, Z)
        call('stft_cov_fused', y, mz)
        call('stft_cov_fused', y, mz, want_cov=False)
        call('step2_cov_fused', X, mw, w_loc)
        call('step2_cov_fused', X, mw, w_loc, want_z=False)
        call('step2_cov_fused_reuse', X, mw, w_loc)
        call('step2_cov_fused_reuse', X, mw, w_loc, want_z=True)
        call('step2_apply_fused', X, w_loc, w_glo)
        call('step2_apply_fused', X, w_loc, w_glo, want_z=True)
        call('step2_apply_istft_fused', X, w_loc, w_glo)
        call('rir_convolve', mkf(3, 40), mkf(3, 2, 10))
        call('rir_convolve', mkf(3, 40), mkf(3, 2, 10), out_len=45)
        call('ism_rir', mkf(2, 3), mkf(2), mkf(2, 1, 3), mkf(2, 4, 3), max_order=3, rir_len=128)
        call('selftest_pk', mkc(8), mkc(8), mkc(8))
        call('selftest_dpp', mk(kind, (64,), np.complex128), mk(kind, (64,), np.complex128))
        call('selftest_room', mkf(256))
        call('selftest_staged_step2', X, mz, w_loc)
        call('selftest_staged_step2', X, mz, w_loc, store_z=False)
        call('selftest_pending_matrices', M)
        call('selftest_pending_matrices', M + K - 1)
        call('selftest_pending_matrices', M + 1)
        # the metrics: stop None / a scalar / one per signal, on all six
        n = 5
        a, b = mkf(n, LS), mkf(n, LS)
        b_eq = mk(kind, (n, LS), f32, fill=1.0)
        stops = (None, 50, np.int64(60), np.array([10, 20, 30, 40, 64]), np.array([10, 20, 30, 40, 64], np.int32))
        bad_stops = (np.array([10, 20, 30]), np.array([10., 20., 30., 40., 64.]), np.array([10, 20, 30, 40, 65]), np.array([4, 20, 30, 40, 64]), 65, 2.5)
        bb, ba = np.ones((3, 9)), np.ones((3, 9))
        refs, ests = mkf(n, 2, LS), mkf(n, 3, 2, LS)
        for stop in stops + bad_stops:
            call('pair_stats', a, b, start=5, stop=stop)
            call('pair_stats', a, a, stop=stop)
            call('band_stats', a, bb, ba, start=5, stop=stop)
            call('band_stats', a, bb, ba, start=5, stop=stop, gate=b)
            call('lag_corr', a, b, -3, 4, start=5, stop=stop)
            call('lag_corr', a, a, 0, 0, stop=stop)
            call('bss_eval', refs, ests, start=5, stop=stop, flen=8)
            call('bss_eval', refs, ests, start=5, stop=stop, flen=8, all_pairs=True, budget_bytes=2000)
            call('bss_estimates', a, b, a, start=5, stop=stop)
            call('stoi', a, b, 16000, start=5, stop=stop)
            call('stoi', a, b, 10000, start=5, stop=stop, budget_bytes=2000, want_kept=True)
        call('pair_stats', mk(kind, (n, LS), f32, fill=1.0), b_eq)                   # equal but distinct objects: two uploads
        call('pair_stats', a, b, start=-1, stop=np.array([10, 20, 30, 40, 64]))
        call('stoi', a, b, 16000, stop=np.array([33]))                                 # stoi broadcasts
        call('stoi', a, b, 16000, stop=[20.5, 30.5, 40.5, 50.5, 60.5])               # ... and truncates
        call('stoi', a, b, 16000, stop=np.array([10, 20]))
        for start in (-1, 65):
            call('stoi', a, b, 16000, start=start)
            call('bss_estimates', a, b, a, start=start)
            call('bss_estimates', a, b, a, start=start, stop=64)
        call('stoi', a, b, 16000.5)
        call('stoi', a, b[:, :-1] if kind == 'np' else mkf(n, LS - 1), 16000)
        call('stoi', mkf(0, LS), mkf(0, LS), 16000)
        call('band_stats', a, bb[:, :8], ba[:, :8])
        call('band_stats', a, bb, ba, gate=mkf(n, LS - 1))
        call('lag_corr', a, mkf(n, LS - 1), 0, 1)
        call('bss_eval', refs, mkf(n, 3, 2, LS - 1))
        call('bss_eval', mkf(n, 0, LS), mkf(n, 3, 0, LS))
        call('bss_estimates', a, mkf(n, LS - 1), a)
        call('bss_estimates', mkf(LS), mkf(LS), mkf(LS))
        call('bss_estimates', mkf(0, LS), mkf(0, LS), mkf(0, LS))
        call('bss_estimates', a, b, a, out=mk('dev', (n, 6, LS - 1)))
        # chunks of 2 over 5 with one host and one device input, both ways round
        other = mk('dev' if kind == 'np' else 'np', (n, 3, 2, LS))
        call('bss_eval', refs, other, flen=8, budget_bytes=2999, stop=np.array([10, 20, 30, 40, 64]))
        call('bss_eval', mk('dev' if kind == 'np' else 'np', (n, 2, LS)), ests, flen=8, budget_bytes=2000)
        other = mk('dev' if kind == 'np' else 'np', (n, LS))
        call('stoi', a, other, 16000, budget_bytes=2999, stop=np.array([10, 20, 30, 40, 64]))
        call('stoi', other, b, 8000, budget_bytes=2000)
        call('bss_eval', refs, ests, budget_bytes=0)                                  # one set per chunk at the least
        lib.per_item = 0                                                               # the "unsupported shape" probe
        call('bss_eval', refs, ests, stop=40)
        call('bss_eval', refs, ests, stop=np.array([10, 20, 30, 40, 64]))
        call('stoi', a, b, 16000, stop=40)
        lib.returns['disco_bss_eval'] = lib.returns['disco_stoi'] = -2
        call('bss_eval', refs, ests)
        call('stoi', a, b, 16000)
        lib.returns.clear()
        lib.per_item = 1000
        # plumbing
        call('to_device', None, f32)
        call('to_device', a, f32)
        call('to_device', mk('dev', (4,), f32), np.float64)
        call('to_device', lib.note_tensor(torch.zeros(4, dtype=torch.float64)), f32)
        call('to_device', lib.note_tensor(torch.zeros(4, 2)), c64)                     # complex64 as its (..., 2) float32 view
        call('to_device', lib.note_tensor(torch.zeros(4, 4))[:, ::2], f32)
        call('to_device', [1, 2, 3], np.int32)
        d = call('empty', (3, 4), f32)
        d.numpy(), d.reshape(4, 3), d.reshape(12).free(), d.free()
        del d
    # configuration
    call('reserve')
    call('reserve', 2)
    call('owned_bytes')
    call('sync')
    call('stage_timing')
    call('stage_timing', False)
    call('stage_report')
    call('set_option', 'room_cov', 1)
    call('get_option', 'room_cov')
    call('set_tuning', 1, 2, 3, 4)
    call('set_z_blocks', 1)
    call('set_lengths', [64, 32])
    call('lengths')
    call('frames')
    kid = call('sibling', 1, first_room=1)
    call('follow', eng, 1, _on=kid)
    call('close', _on=kid)
    call('set_lengths', [64.5, 32])
    call('set_lengths', None)
    call('lengths')
    call('set_node_shard', 1, 1)
    call('cov_masked', mk('np', (R, 1, T, F, M), c64), mk('np', (R, 1, T, F)))
    call('gevd_mwf_r1_pending', M)
    kid = call('sibling', 1)
    call('close', _on=kid)
    del kid
    lib.returns['disco_reserve'] = -1
    call('reserve')
    del lib.returns['disco_reserve']
    # Methods newer than the first trees this script compared go last: every allocation number before this point is then the same in a
    # parent that lacks them and in a change that has them.  The section is marked: when one tree lacks a method of it, the comparison leaves
    # the section out of both traces (`comparable`), and the change's own trace of it still answers for its pointers and its leaks.
    lib.trace.append(['section', 'newer methods'])
    for kind in KINDS:
        mkf = lambda *shape: mk(kind, shape, np.float32)
        n = 5
        a, b = mkf(n, LS), mkf(n, LS)
        for stop in (None, 50, np.array([10, 20, 30, 40, 64]), np.array([10, 20, 30]), 65):
            call('estoi', a, b, 16000, start=5, stop=stop)
            call('estoi', a, b, 10000, start=5, stop=stop, budget_bytes=2000, want_kept=True)
        call('estoi', a, mkf(n, LS - 1), 16000)
        call('estoi', mk('dev' if kind == 'np' else 'np', (n, LS)), b, 8000, budget_bytes=2999, stop=np.array([10, 20, 30, 40, 64]))
        lib.per_item = 0
        call('estoi', a, b, 16000, stop=40)
        lib.per_item = 1000
        lib.returns['disco_estoi'] = -2
        call('estoi', a, b, 16000)
        lib.returns.clear()
        X, Y = mkf(3, 15, 100), mkf(3, 15, 100)
        call('estoi_bands', X, Y)
        call('estoi_bands', X, Y, frames=np.array([29, 30, 100]))
        call('estoi_bands', X, Y, frames=np.array([29, 30, 101]))
        call('estoi_bands', X, Y, frames=np.array([29., 30., 40.]))
        call('estoi_bands', X, mkf(3, 15, 99))
        call('estoi_bands', mkf(3, 14, 100), mkf(3, 14, 100))
        lib.returns['disco_estoi_bands'] = -1
        call('estoi_bands', X, Y)
        lib.returns.clear()
        del a, b, X, Y
    lib.trace.append(['section', 'end'])
    # every temporary is gone once the results are: what is live now belongs to the engine's cache of resampling taps
    gc.collect()
    cached = {lib._alloc_of(v[1].ptr) for v in getattr(eng, '_stoi_taps', {}).values()}
    leaked = sorted(lib.live - cached)
    call('close')
    lib.returns['disco_create'] = -1
    covered.add('__init__')
    try:
        Engine(rooms=1, nodes=1, mics=1, length=LS, n_fft=16, lib=lib)
    except Exception as e:
        errors.append((len(lib.trace), '__init__', type(e).__name__, str(e)))
    lib.returns.clear()
    public = {nm for nm in vars(Engine) if not nm.startswith('_') and (callable(getattr(Engine, nm)) or isinstance(getattr(Engine, nm), property))}
    missing = sorted(public - covered)
    return errors, sorted(covered), missing, leaked, sorted(absent)


def dump(tree):
    engine, _lib = load_engine(tree)
    lib = RecordingLib(_lib.PROTOTYPES)
    errors, covered, missing, leaked, absent = run_script(engine, lib)
    late = [f for f in lib.frees if f[2] is not None and f[2] >= f[1]]
    return dict(trace=lib.trace, errors=errors, covered=covered, missing=missing, leaked=leaked, absent=absent,
                violations=lib.violations + [f'free {f}' for f in late],
                allocations=len(lib.starts), frees=len(lib.frees), engine_lines=len(open(engine.__file__).read().splitlines()))


def time_calls(tree, n_calls=10000):
    """Seconds for `n_calls` of tango_enhance on DevBuf inputs with out= given, against the stand-in."""
    engine, _lib = load_engine(tree)
    lib = RecordingLib(_lib.PROTOTYPES)
    eng = engine.Engine(rooms=R, nodes=K, mics=M, length=LS, n_fft=16, lib=lib)
    y, mz, out = eng.empty((R, K, M, LS), np.float32), eng.empty((R, K, eng.T, eng.F), np.float32), eng.empty((R, K, LS), np.float32)
    for _ in range(1000):
        eng.tango_enhance(y, mz, out=out)
    del lib.trace[:]
    gc.collect()
    gc.disable()
    t0 = time.perf_counter()
    for _ in range(n_calls):
        eng.tango_enhance(y, mz, out=out)
    dt = time.perf_counter() - t0
    gc.enable()
    return dt


def child(mode, tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode, tree], check=True, capture_output=True, text=True).stdout
    return json.loads(out.splitlines()[-1])


def without_frees(trace):
    return [e for e in trace if e[0] != 'disco_dev_free']


def without_section(trace):
    """The trace without what lies between the markers of the section of newer methods."""
    out, skip = [], False
    for e in trace:
        if e[0] == 'section':
            skip = e[1] != 'end'
        elif not skip:
            out.append(e)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('trees', nargs='*', help='PARENT_TREE CHANGE_TREE')
    ap.add_argument('--dump', metavar='TREE')
    ap.add_argument('--time-one', metavar='TREE')
    ap.add_argument('--time', action='store_true', help='five alternated repetitions of 10 000 tango_enhance calls per tree')
    ap.add_argument('--out', help='write the verdict here as well')
    a = ap.parse_args()
    if a.dump:
        print(json.dumps(dump(a.dump)))
        return 0
    if a.time_one:
        print(json.dumps(time_calls(a.time_one)))
        return 0
    parent, change = a.trees
    if a.time:
        t = {parent: [], change: []}
        for _ in range(5):
            for tree in (parent, change):
                t[tree].append(child('--time-one', tree))
        mp, mc = statistics.median(t[parent]), statistics.median(t[change])
        spread = max(t[parent]) - min(t[parent])
        print('microseconds per tango_enhance call (DevBuf inputs, out= given), five alternated repetitions of 10 000 calls')
        for nm, tree in (('parent', parent), ('change', change)):
            print(f'  {nm}: ' + ', '.join(f'{v * 100:.2f}' for v in t[tree]) + f'   median {statistics.median(t[tree]) * 100:.2f}')
        print(f'  change - parent = {(mc - mp) * 100:+.2f}, the parent\'s max - min spread {spread * 100:.2f}: ' + ('within' if mc - mp <= spread else 'BEYOND') + ' the spread')
        return 0 if mc - mp <= spread else 1
    p, c = child('--dump', parent), child('--dump', change)
    tp, tc = without_frees(p['trace']), without_frees(c['trace'])
    one_sided = sorted(set(p['absent']) ^ set(c['absent']))               # methods only one tree has: their section is left out of both
    ep, ec = p['errors'], c['errors']
    if one_sided:
        tp, tc = without_section(tp), without_section(tc)
        ep, ec = ([e[1:] for e in errs if e[1] not in one_sided] for errs in (ep, ec))       # positions shift with the section: names and messages in order
    lines = []
    first = next((i for i, (x, y) in enumerate(zip(tp, tc)) if x != y), None if len(tp) == len(tc) else min(len(tp), len(tc)))
    same_errors = ep == ec
    ok = first is None and same_errors and not c['violations'] and not c['leaked'] and not c['missing'] and not p['violations']
    lines.append('engine call trace: parent and change ' + ('IDENTICAL' if first is None and same_errors else 'DIFFER') +
                 ' (normalised traces call for call, the positions of disco_dev_free apart; raised exceptions by type and message)')
    lines.append(f'calls compared: {len(tc)} entries of the change against {len(tp)} of the parent, {sum(e[0].startswith("disco_") for e in tc)} of them library calls, '
                 f'{sum(e[0] == "step" for e in tc)} scripted method calls; exceptions compared: {len(c["errors"])} against {len(p["errors"])}')
    if one_sided:
        lines.append(f'methods only one tree has: {", ".join(one_sided)} -- the section of newer methods is left out of both traces; the change ran it '
                     f'({sum(e[0] == "step" for e in c["trace"]) - sum(e[0] == "step" for e in tc)} scripted calls) and its pointers and leaks are counted below')
    if first is not None:
        lines.append(f'first difference at entry {first}: parent {tp[first] if first < len(tp) else None}, change {tc[first] if first < len(tc) else None}')
        lines.append('  in step: ' + str(next((e for e in reversed(tc[:first + 1]) if e[0] == 'step'), None)))
    if not same_errors:
        lines.append('first differing exception: ' + str(next(((x, y) for x, y in zip(p['errors'] + [None], c['errors'] + [None]) if x != y), None)))
    for nm, d in (('parent', p), ('change', c)):
        lines.append(f'{nm}: {d["allocations"]} allocations, {d["frees"]} frees; pointers into freed allocations / double frees: {len(d["violations"])}; '
                     f'temporaries alive at the end: {len(d["leaked"])}; engine.py {d["engine_lines"]} lines')
        lines += ['  ' + v for v in d['violations'][:10]]
    lines.append(f'public methods of Engine not covered: {c["missing"] or "none"}')
    lines.append('methods covered (Engine, and push / frames_of of the online stream): ' + ', '.join(c['covered']))
    lines.append('verdict: ' + ('PASS' if ok else 'FAIL'))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
