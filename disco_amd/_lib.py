"""ctypes binding of libdisco_hip.so (the C ABI of include/disco_hip.h).

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible, `load()` / `Engine`
raise.  (tests/ may bind the same prototypes onto the hipemu *test* build through `bind`; the package
itself never does.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DISCO_HIP_LIB', os.path.join(_HERE, 'lib', 'libdisco_hip.so'))   # override: A/B of kernel builds

E_ARG, E_UNSUPPORTED, E_HIP_BASE = -1, -2, -1000
MASK_TYPES = {'irm': 0, 'ibm': 1, 'iam': 2}
PAD_MODES = {'reflect': 0, 'constant': 1}
FLAG_STAGED_STEP2 = 1
FLAG_LAZY_SCRATCH = 2
FLAG_NO_CHILDREN = 4
SEG_SNR_MAX_WIN = 2048                  # DISCO_SEG_SNR_MAX_WIN: the longest window disco_seg_snr takes
REVERB_MAX_RIR = 8192                   # DISCO_REVERB_MAX_RIR: the longest response disco_rir_split / disco_reverb_energies take
RECON_LOSS_WS_BYTES = 16384             # DISCO_RECON_LOSS_WS_BYTES: the workspace disco_recon_loss never needs more than
ESTOI_SEGS = 64                # DISCO_ESTOI_SEGS of include/disco_hip.h: segments one workgroup of k_estoi_corr owns


class DiscoCfg(C.Structure):
    """struct disco_cfg (include/disco_hip.h); mirrors the constants of tango.py:28-38."""
    _fields_ = [('rooms', C.c_int32), ('nodes', C.c_int32), ('mics', C.c_int32), ('length', C.c_int32),
                ('n_fft', C.c_int32), ('hop', C.c_int32), ('ref_mic', C.c_int32), ('mask_type', C.c_int32),
                ('mask_pow', C.c_int32), ('mask_bin_thr_db', C.c_float), ('mu', C.c_float),
                ('pad_mode', C.c_int32), ('device', C.c_int32), ('flags', C.c_int32), ('reserved', C.c_int32 * 2)]


class DiscoRefOutputs(C.Structure):
    """struct disco_ref_outputs: device pointers of the nine returns of offline_tango (NULL = not wanted)."""
    _fields_ = [(nm, C.c_void_p) for nm in ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w')]


class DiscoOnlineCompanion(C.Structure):
    """struct disco_online_companion: one companion of disco_online_mwf_ref (X, Z or NULL, out)."""
    _fields_ = [('X', C.c_void_p), ('Z', C.c_void_p), ('out', C.c_void_p)]


MASK_FOR_Z = {'local': 0, None: 1, 'distant': 2, 'compressed': 3, 'use_oracle_refs': 4, 'use_oracle_zs': 5, 'previous': 6}

# name -> (restype, argtypes); every symbol the header declares
_vp, _i64, _int, _sz, _f = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_float
PROTOTYPES = {
    'disco_version': (C.c_char_p, []),
    'disco_create': (_int, [C.POINTER(_vp), C.POINTER(DiscoCfg)]),
    'disco_destroy': (None, [_vp]),
    'disco_last_error': (C.c_char_p, [_vp]),
    'disco_n_frames': (_int, [_vp]),
    'disco_n_freq': (_int, [_vp]),
    'disco_workspace_bytes': (_sz, [_vp]),
    'disco_reserve': (_int, [_vp, _int]),
    'disco_owned_bytes': (_sz, [_vp]),
    'disco_set_node_shard': (_int, [_vp, _int, _int]),
    'disco_set_z_blocks': (_int, [_vp, _int]),
    'disco_set_lengths': (_int, [_vp, _vp, _int]),
    'disco_set_tuning': (_int, [_vp, _int, _int, _int, _int]),
    'disco_set_option': (_int, [_vp, C.c_char_p, _int]),
    'disco_get_option': (_int, [_vp, C.c_char_p, C.POINTER(_int)]),
    'disco_stage_timing': (_int, [_vp, _int]),
    'disco_stage_report': (_int, [_vp, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int64), _int]),
    'disco_dev_alloc': (_int, [_vp, _sz, C.POINTER(_vp)]),
    'disco_dev_free': (_int, [_vp, _vp]),
    'disco_h2d': (_int, [_vp, _vp, _vp, _sz, _vp]),
    'disco_d2h': (_int, [_vp, _vp, _vp, _sz, _vp]),
    'disco_sync': (_int, [_vp, _vp]),
    'disco_stft': (_int, [_vp, _vp, _i64, _int, _vp, _vp]),
    'disco_istft': (_int, [_vp, _vp, _i64, _vp, _vp]),
    'disco_tf_mask': (_int, [_vp, _vp, _vp, _i64, _int, _int, _f, _vp, _vp]),
    'disco_mask_oracle': (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    'disco_cov_masked': (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    'disco_gevd_mwf_r1': (_int, [_vp, _vp, _vp, _i64, _int, _f, _vp, _vp, _vp]),
    'disco_gevd_mwf': (_int, [_vp, _vp, _vp, _i64, _int, _int, _f, _vp, _vp, _vp]),
    'disco_mwf_filter': (_int, [_vp, _vp, _vp, _i64, _int, _f, _int, _vp, _vp]),
    'disco_gevd_mwf_r1_pending': (_int, [_vp, _f, _vp, _vp, _vp]),
    'disco_apply': (_int, [_vp, _vp, _vp, _vp, _int, _int, _vp, _vp]),
    'disco_noise_residual': (_int, [_vp, _vp, _vp, _vp, _vp]),
    'disco_filter_head': (_int, [_vp, _vp, _int, _vp, _vp]),
    'disco_stft_cov_fused': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_step2_cov_fused': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_step2_cov_fused_reuse': (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_step2_apply_fused': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_step2_apply_istft_fused': (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_apply_istft_fused': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_tango_enhance': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'disco_mask_ivad': (_int, [_vp, _vp, _i64, _vp, _vp]),
    'disco_rir_convolve': (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _int, _vp]),
    'disco_ism_rir': (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _f, _f, _vp, _int, _vp]),
    'disco_vad_samples': (_int, [_vp, _vp, _i64, _i64, _vp, _int, _int, _f, _int, _vp, _vp]),
    'disco_mix_scaled': (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _vp, _vp]),
    'disco_source_mix': (_int, [_vp, _vp, _int, _i64, _i64, _vp, _int, _vp, _vp, _vp, _vp, _vp]),
    'disco_source_masks': (_int, [_vp, _vp, _int, _i64, _vp, _vp, _vp]),
    'disco_noise_from_signal': (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    'disco_affine_segment': (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp]),
    'disco_gru_gates':(_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _int, _vp]),
    'disco_gru_gates_train': (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp]),
    'disco_gru_gates_backward': (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _int, _vp]),
    'disco_recon_loss': (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _sz, _vp]),
    'disco_recon_loss_grad': (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'disco_train_batch': (_int, [_vp, _vp, _int, _i64, _int, _int, _vp, _vp, _i64, _int, _int, _vp, _vp, _vp]),
    'disco_bank_fill': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, _vp, _i64, _int, _i64, _vp]),
    'disco_maxpool_last4': (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    'disco_conv3x3_pool4': (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp]),
    'disco_crnn_features': (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, C.c_float, C.c_float, _vp, _vp]),
    'disco_crnn_windows': (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp]),
    'disco_crnn_features_rooms': (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, C.c_float, C.c_float, _vp, _vp, _vp]),
    'disco_crnn_windows_rooms': (_int, [_vp, _vp, _i64, _int, _int, _int, _int, _int, _vp, _vp, _vp, _i64, _vp]),
    'disco_crnn_expand_rows': (_int, [_vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _vp, _vp]),
    'disco_pair_stats': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp]),
    'disco_band_stats': (_int, [_vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _int, _vp, _vp]),
    'disco_band_stats_gated': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp, _vp, _int, _vp, _vp]),
    'disco_pair_stats_spans': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _vp]),
    'disco_band_stats_spans': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _int, _vp, _vp]),
    'disco_seg_snr': (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _int, _int, _f, _f, _vp, _vp]),
    'disco_rir_split': (_int, [_vp, _vp, _i64, _int, _int, _vp, _vp, _vp]),
    'disco_reverb_energies': (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    'disco_lag_corr_workspace_bytes': (_sz, [_vp, _i64, _i64, _int]),
    'disco_lag_corr': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _int, _int, _vp, _vp, _sz, _vp]),
    'disco_lag_corr_spans': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _int, _int, _vp, _vp, _sz, _vp]),
    'disco_bss_workspace_bytes': (_sz, [_vp, _i64, _int, _int, _i64]),
    'disco_bss_eval': (_int, [_vp, _vp, _vp, _i64, _int, _int, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    'disco_bss_eval_spans': (_int, [_vp, _vp, _vp, _i64, _int, _int, _i64, _int, _vp, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    'disco_bss_estimates': (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp, _vp]),
    'disco_stoi_workspace_bytes': (_sz, [_vp, _i64, _i64, _int, _int, _int]),
    'disco_stoi': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _int, _int, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    'disco_estoi_workspace_bytes': (_sz, [_vp, _i64, _i64, _int, _int, _int]),
    'disco_estoi': (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _int, _int, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    'disco_estoi_bands': (_int, [_vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    'disco_reference_workspace_bytes': (_sz, [_vp]),
    'disco_tango_reference': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, C.POINTER(DiscoRefOutputs), _vp, _sz, _vp]),
    'disco_tango_enhance_iterated': (_int, [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    'disco_online_mwf': (_int, [_vp, _vp, _vp, _vp, _int, _f, _f, _int, _f, _vp, _vp, _vp]),
    'disco_selftest_stream': (_int, [_vp, _vp, _vp, _i64, _int, _vp]),
    'disco_selftest_pk': (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'disco_selftest_dpp': (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'disco_selftest_room': (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    'disco_selftest_stft_cov_packed': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'disco_selftest_step2_cov_packed': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    'disco_selftest_staged_step2': (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp]),
    'disco_selftest_pending_matrices': (_int, [_vp, _vp, _vp, _vp]),
    'disco_tango_online': (_int, [_vp, _vp, _vp, _vp, _f, _int, _f, _vp, _vp, _vp, _vp, _sz, _vp]),
    'disco_online_mwf_ref': (_int, [_vp, _vp, _vp, _vp, _int, _f, _f, _int, _f, _vp, _vp, C.POINTER(DiscoOnlineCompanion), _int, _vp]),
    'disco_online_reference_workspace_bytes': (_sz, [_vp]),
    'disco_tango_online_reference': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f, _int, _f, C.POINTER(DiscoRefOutputs), _vp, _vp, _sz, _vp]),
    'disco_online_state_bytes': (_sz, [_vp]),
    'disco_online_stream_workspace_bytes': (_sz, [_vp, _int]),
    'disco_tango_online_stream': (_int, [_vp, _vp, _int, _vp, _vp, _f, _int, _f, _i64, _int, _vp, _vp, _vp, _sz, _vp]),
}


def bind(cdll):
    """Attach the prototypes of include/disco_hip.h to a loaded library; raises AttributeError on a missing symbol."""
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(cdll, name)
        fn.restype = res
        fn.argtypes = args
    return cdll


_lib = None
_gfx950 = None      # what load() itself opened: the only library the package ever loads


def takes_host_memory():
    """True where a test has put a library of its own in `_lib` (the hipemu build, whose "device" pointers are host pointers).  The training
    wrappers (dnn/losses.py, dnn/crnn.py) then drive their kernels on CPU tensors too; with the gfx950 library, or none, CPU tensors take the
    torch expressions."""
    return _lib is not None and _lib is not _gfx950


def load():
    """Load the gfx950 library.  Fails loudly -- there is no other implementation to fall back to."""
    global _lib, _gfx950
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950).  disco_amd has no CPU path.')
        # One HIP / HSA runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64, and a process
        # that initialises the system copy first (through this library) and torch's afterwards ends with torch reporting
        # "No HIP GPUs are available".  Loaded first, torch's copy carries the soname this library needs, so the dynamic
        # loader binds both to it -- which is also what makes zero-copy use of torch tensors legitimate.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _gfx950 = bind(C.CDLL(LIB_PATH))
    return _lib
