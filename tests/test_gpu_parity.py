"""Parity of the HIP path (through the C ABI of libdisco_hip.so, on a real MI355X) with the CPU oracle.

Tolerances: the north star asks for 1e-4 relative on the outputs; stage kernels are held to fp32-rounding
class bounds (see tests/parity_checks.py).  Relative error = ||a-b||_2 / ||b||_2 per (room, node) signal."""
import os

import numpy as np
import pytest

import parity_checks as pc
from disco_amd import _lib, synth
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_native_library_is_loaded(make_engine):
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    assert b'gfx950' in eng.lib.disco_version()
    maps = open('/proc/self/maps').read()
    assert 'libdisco_hip.so' in maps


@pytest.mark.gpu
def test_pk_instruction_forms(make_engine):
    pc.check_pk_selftest(make_engine)


@pytest.mark.gpu
def test_room_pass_instruction_forms(make_engine):
    """LDS-DMA loads and permlane swaps of csrc/k_room.h against plain statements, bit for bit (round-4 VERDICT weak 7)."""
    print(pc.check_room_selftest(make_engine))


def test_dpp_instruction_forms(make_engine):
    print(pc.check_dpp_selftest(make_engine, n=4096))


@pytest.mark.parametrize('n_fft,L,chans', [(512, 1500, 3), (512, 160000, 4), (1024, 2600, 1), (1024, 40000, 8), (1024, 30000, 3),
                                           (512, 20000, 5), (512, 45000, 8), (1024, 21000, 4), (1024, 30000, 7)])
@pytest.mark.parametrize('pad_mode', ['reflect', 'constant'])
def test_stft(make_engine, n_fft, L, chans, pad_mode):
    pc.check_stft(make_engine, n_sig=3, chans=chans, L=L, n_fft=n_fft, pad_mode=pad_mode)


@pytest.mark.parametrize('n_fft,L', [(512, 2048), (512, 2100), (512, 160000), (1024, 4500), (1024, 160000)])
def test_istft(make_engine, n_fft, L):
    pc.check_istft(make_engine, n_sig=3, L=L, n_fft=n_fft)


def test_masks(make_engine):
    pc.check_masks(make_engine, L=20000)


@pytest.mark.parametrize('R,K,M,same_z,mask_remote', [(2, 2, 2, True, True), (3, 3, 2, False, False), (5, 1, 4, True, True),
                                                     (4, 4, 4, True, True), (2, 2, 5, True, True), (1, 1, 8, True, True),
                                                     (2, 5, 3, False, True), (2, 8, 8, True, True), (1, 3, 7, False, False), (2, 6, 5, True, True),
                                                     (2, 6, 4, True, True), (1, 13, 4, True, True), (2, 8, 2, True, True), (1, 15, 2, True, True),
                                                     (1, 9, 8, True, True), (2, 2, 8, True, True)])
def test_cov_solve_apply(make_engine, R, K, M, same_z, mask_remote):
    pc.check_cov_solve_apply(make_engine, R=R, K=K, M=M, L=16000, same_z=same_z, mask_remote=mask_remote)


@pytest.mark.parametrize('R,K,M,L,n_fft', [(3, 4, 4, 160000, 512), (2, 2, 3, 30000, 512), (2, 1, 8, 20000, 512), (2, 2, 2, 50000, 1024),
                                          (1, 1, 1, 5000, 512), (2, 2, 8, 160000, 1024), (1, 3, 7, 40000, 1024)])
def test_stft_cov_fused(make_engine, R, K, M, L, n_fft):
    pc.check_stft_cov_fused(make_engine, R=R, K=K, M=M, L=L, n_fft=n_fft)


@pytest.mark.parametrize('R,K,M', [(3, 4, 4), (2, 2, 2), (2, 3, 2), (2, 1, 3), (1, 5, 4), (2, 8, 1), (2, 2, 7)])
def test_step2_fused(make_engine, R, K, M):
    pc.check_step2_fused(make_engine, R=R, K=K, M=M, L=16000)


@pytest.mark.parametrize('R,K,M', [(3, 4, 4), (2, 2, 2), (1, 5, 3), (2, 3, 5)])
def test_step2_reuse(make_engine, R, K, M):
    pc.check_step2_reuse(make_engine, R=R, K=K, M=M, L=40000)


@pytest.mark.parametrize('start', [0, 5000])
def test_metrics(make_engine, golden_dir, start):
    pc.check_metrics(make_engine, golden_dir, start=start)


@pytest.mark.parametrize('n_sig,n_ch,Ld,Lh,out_len', [(3, 4, 20000, 4096, None), (2, 16, 160000, 4096, None), (2, 2, 5000, 8192, 14000),
                                                      (1, 1, 700, 100, 513), (5, 3, 9000, 5000, 9000)])
def test_rir_convolve(make_engine, n_sig, n_ch, Ld, Lh, out_len):
    pc.check_rir_convolve(make_engine, n_sig=n_sig, n_ch=n_ch, Ld=Ld, Lh=Lh, out_len=out_len)


def test_synth_rooms_through_rir_convolve(make_engine):
    """The bench's room generator with its source images formed by the library's own RIR convolution (disco_rir_convolve)
    against the same generator on torch.fft: the same rooms to float32 rounding, at the bench's clip length and RIR length."""
    import torch
    from disco_amd import synth
    eng = make_engine(rooms=1, nodes=1, mics=1, length=1024)
    a = synth.make_rooms_torch(2, K=2, M=4, L=160000, device='cuda:0', ref_only_sn=False)
    b = synth.make_rooms_torch(2, K=2, M=4, L=160000, device='cuda:0', ref_only_sn=False, engine=eng)
    for x, y_ in zip(a, b):
        e = float((x - y_).norm() / x.norm())
        assert e < 2e-6, e


def test_ism_rir_pinned(make_engine):
    """hand-derived order-1 shoebox, mirror construction to order 3, reciprocity at order 20, per-reflection gain, decay vs room_setups.py:92"""
    print(pc.check_ism_pinned_hip(make_engine))


@pytest.mark.parametrize('max_order,rir_len', [(6, 4096), (20, 8192)])
def test_ism_rir(make_engine, max_order, rir_len):
    pc.check_ism_rir(make_engine, n_room=2, S=2, Q=2, max_order=max_order, rir_len=rir_len)


def test_solver_singular_noise(make_engine):
    pc.check_solver_singular_noise(make_engine)


def test_ivad(make_engine, golden_dir):
    pc.check_ivad(make_engine, golden_dir)


@pytest.mark.parametrize('R,K,M,L,n_fft,U', [(3, 4, 4, 40960, 512, 1), (2, 3, 2, 20480, 512, 4), (1, 2, 8, 40960, 1024, 3), (2, 1, 4, 15360, 512, 2)])
def test_online_stream_equals_whole_clip(make_engine, R, K, M, L, n_fft, U):
    """disco_tango_online_stream: N chunks == one whole-clip call of disco_tango_online, bit for bit (state in / state out; the transform's
    and the overlap-add's halves carried across chunks)."""
    print(pc.check_online_stream(make_engine, R=R, K=K, M=M, L=L, n_fft=n_fft, update_every=U))


def test_online_golden(make_engine, golden_dir):
    pc.check_online_golden(make_engine, golden_dir)


@pytest.mark.parametrize('R,K,M,L,n_fft,U', [(2, 4, 4, 12000, 512, 1), (2, 3, 2, 20000, 512, 4), (1, 1, 4, 16000, 512, 1),
                                             (1, 2, 3, 30000, 1024, 2), (1, 5, 1, 8000, 512, 1)])
def test_online_mwf(make_engine, R, K, M, L, n_fft, U):
    pc.check_online_mwf(make_engine, R=R, K=K, M=M, L=L, n_fft=n_fft, update_every=U)


@pytest.mark.parametrize('K,M,world', [(4, 4, 2), (4, 2, 4), (6, 2, 3), (4, 4, 4), (2, 4, 2), (3, 4, 3)])
def test_node_sharded_equals_single_gpu(make_engine, K, M, world):
    """(the 4-mic shapes end in ONE filter + iSTFT pass on the gathered z: disco_apply_istft_fused)"""
    pc.check_node_sharded(make_engine, R=2, K=K, M=M, L=30000, world=world)


@pytest.mark.parametrize('K,M,n_fft,L,world,R', [(4, 4, 512, 42000, 2, 3), (4, 4, 512, 160000, 4, 2), (2, 4, 512, 20000, 2, 5), (3, 4, 1024, 30000, 3, 2),
                                                  (4, 4, 512, 9000, 1, 2), (4, 8, 512, 20000, 2, 2), (8, 8, 1024, 30000, 4, 1), (4, 4, 1024, 600, 2, 1)])
def test_apply_istft_sharded(make_engine, K, M, n_fft, L, world, R):
    """disco_apply_istft_fused on node shards (k_apply_istft_wide with the shard's nodes and the gathered z in rank-major blocks) against
    disco_apply + disco_istft: the filtered spectra bit for bit, the samples to rounding; full-length clips, several chunks per node, a clip
    shorter than a frame, the unsharded context."""
    print(pc.check_apply_istft_sharded(make_engine, K=K, M=M, L=L, n_fft=n_fft, R=R, world=world))


def test_solver_vs_reference_golden(make_engine, golden_dir):
    pc.check_solver_vs_reference_golden(make_engine, golden_dir)


def test_solver_sizes_up_to_16(make_engine):
    """P = 1..16 (C5 needs 15): HIP float64 solver vs numpy eigh closed form."""
    pc.check_solver_sizes(make_engine)


def test_solver_small_gap(make_engine):
    print(pc.check_solver_small_gap(make_engine))


def test_solver_routes_dpp_vs_lds(make_engine):
    print(pc.check_solver_routes(make_engine, sizes=(9, 10, 11, 12, 13, 14, 15, 16), n=4099))


def test_solver_routes_thread_vs_group(make_engine):
    """5 <= P <= 8: one thread per pencil (default) against the LDS group solver (option "solve_thread" 0): full matrices, and both loaders
    through the partial sums of a covariance call."""
    print(pc.check_solver_routes(make_engine, sizes=(5, 6, 7, 8), option='solve_thread'))
    for M in (5, 6, 7, 8):
        for thread in (0, 1):
            print(M, thread, pc.check_cov_solve_apply(make_engine, R=2, K=1, M=M, L=16384, options={'solve_thread': thread}))


def test_solver_degenerate_inputs(make_engine):
    pc.check_solver_degenerate(make_engine)


@pytest.mark.parametrize('sizes,option,value', [((1, 2, 3, 4), None, None), ((5, 6, 7, 8), 'solve_thread', 1), ((5, 6, 7, 8), 'solve_thread', 0),
                                                (tuple(range(9, 17)), 'solve_dpp', 1), (tuple(range(9, 17)), 'solve_dpp', 0)])
def test_solver_indefinite(make_engine, sizes, option, value):
    """Indefinite pencils (Rxx = Ryy - Rnn): the top generalized eigenpair, clamped, on every route of the rank-1 solve."""
    print(pc.check_solver_indefinite(make_engine, sizes=sizes, option=option, value=value))


def test_mwf_variants(make_engine):
    """disco_mwf_filter ('mwf', 'r1-mwf'): every P, full and ragged blocks, mu != 1, PSD / indefinite / negative Rxx."""
    print(pc.check_mwf_variants(make_engine))


@pytest.mark.parametrize('K,M,L,n_fft,staged', [(4, 4, 160000, 512, False), (4, 4, 160000, 512, True), (1, 4, 160000, 512, False),
                                                (2, 3, 20000, 512, False), (2, 2, 40000, 1024, False), (3, 2, 30000, 512, True),
                                                (8, 8, 40000, 1024, False)])
def test_tango_end_to_end_vs_oracle(make_engine, K, M, L, n_fft, staged):
    """Full path on synthetic rooms (SURVEY 8d generator) vs the float64 oracle; bar: 1e-4 relative.
    staged=False: step 2 on the in-register z exchange (default); True: z materialised, staged kernels."""
    y, s, n = synth.make_rooms_numpy(2, K=K, M=M, L=L)
    errs = pc.check_tango_end_to_end(make_engine, y, s, n, n_fft=n_fft, tol=1e-4, staged_step2=staged)
    print(K, M, L, n_fft, staged, errs)


# The launch geometry bench.py's headline run takes (R*K = 4000: 40 frames per STFT wave -> 4 chunks with a short last one -- 80 frames and
# 2 chunks until late round 5 --, single-chunk covariances, 64 frame pairs per filter+iSTFT workgroup), pinned on small batches; plus
# geometries whose tails fall differently (empty waves, one-frame last chunks).
@pytest.mark.parametrize('R,K,M,L,n_fft,tuning', [(2, 4, 4, 160000, 512, (40, 1, 1, 64)), (2, 4, 4, 160000, 512, (80, 1, 1, 64)), (1, 4, 4, 160000, 512, (80, 1, 1, 64)),
                                                 (2, 4, 4, 25700, 512, (80, 1, 1, 64)), (2, 2, 3, 160000, 512, (79, 1, 1, 63)),
                                                 (2, 4, 4, 82000, 512, (40, 2, 3, 20)), (1, 2, 2, 80000, 1024, (80, 1, 1, 0)),
                                                 (2, 1, 4, 160000, 512, (80, 1, 1, 64))])
def test_tango_bench_geometry(make_engine, R, K, M, L, n_fft, tuning):
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    errs = pc.check_tango_end_to_end(make_engine, y, s, n, n_fft=n_fft, tol=1e-4, tuning=tuning)
    print(errs)


@pytest.mark.parametrize('R,K,M,L,tuning', [(2, 4, 4, 160000, (80, 1, 1, 64)), (2, 2, 3, 41000, None), (1, 3, 2, 25700, (80, 1, 1, 5)),
                                            (2, 4, 1, 30000, None)])
def test_enhanced_only_geometries(make_engine, R, K, M, L, tuning):
    """The step-2 filter + iSTFT kernel of the enhanced-only call (the spectra read back, yf on chip) at the bench geometry and at
    ragged ones: odd and even mic counts, signals that end inside a frame pair, one-pair workgroups."""
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    errs = pc.check_tango_end_to_end(make_engine, y, s, n, tol=1e-4, tuning=tuning)
    print(errs)


def test_large_batch_default_geometry(make_engine):
    """R*K = 2048 rooms-nodes of a SHORT signal: the batch-size heuristics themselves pick the large-batch geometry
    (long runs, single chunks); 4 sampled rooms are checked against the float64 oracle, the rest against the same rooms
    computed in a small batch (batch independence)."""
    R, K, M, L = 512, 4, 4, 25600
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    m = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, eng.T, eng.F)
    out = eng.tango_enhance(y, m, want_z=False, want_yf=False)[0].numpy()
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    for r in (0, 137, 300, 511):
        o = to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
        for k in range(K):
            ref = so.istft(o['yf'][k], L, work_dtype=np.float64)
            assert pc.relerr(out[r, k], ref) < 1e-4, (r, k)
    sub = slice(200, 204)
    eng2 = make_engine(rooms=4, nodes=K, mics=M, length=L)
    m2 = eng2.mask_oracle(s[sub, :, 0].reshape(4 * K, L), n[sub, :, 0].reshape(4 * K, L)).reshape(4, K, eng2.T, eng2.F)
    out2 = eng2.tango_enhance(y[sub], m2, want_z=False, want_yf=False)[0].numpy()
    assert pc.relerr(out[sub], out2) < 2e-5


def test_c2_single_node_config(make_engine):
    """BASELINE.json configs[1] (C2) shape: single node x 4 mics, many rooms; output = iSTFT(z) (K = 1)."""
    y, s, n = synth.make_rooms_numpy(3, K=1, M=4, L=48000)
    errs = pc.check_tango_end_to_end(make_engine, y, s, n, tol=1e-4)
    print('C2', errs)


@pytest.mark.parametrize('K,M,L,n_fft,iters', [(3, 2, 30000, 512, 2), (8, 8, 30720, 1024, 2), (2, 2, 20000, 512, 3)])
def test_iterated_danse_extension(make_engine, K, M, L, n_fft, iters):
    """BASELINE.json configs[4] (C5): DANSE-style extra iterations of step 2.  This is an EXTENSION: the reference is
    strictly two-step (tango.py:1-2), so there is no reference parity; the check is against the oracle's restatement
    of the same definition (z_k <- w_glo,k[:M]^H y_k)."""
    print(pc.check_iterated_outputs(make_engine, K, M, L, n_fft, iters))


def test_c5_full_length_rooms(make_engine):
    """BASELINE.json configs[4] at full shape and length (8 x 8, 1024-point, L = 160000, 2 iterations), rooms 0 / 6 / 64 / 100 / 141 / 199 of
    the bench's batch, 1e-4 against the float64 oracle."""
    print(pc.check_c5_full_length(make_engine))


@pytest.mark.parametrize('scene', ['k2m2', 'k4m4'])
def test_tango_vs_reference_golden(make_engine, golden_dir, scene):
    """HIP path against outputs of the REFERENCE'S OWN offline_tango on the short scenes (tests/golden/tango_ref_*.npz, 17-25
    frames), per (node, bin): 1e-4 against the reference on the bins whose sensitivity kappa <= 2e3, 1e-4 against the float64
    restatement on all bins."""
    print(pc.check_short_reference_scene_per_bin(make_engine, golden_dir, scene))


@pytest.mark.parametrize('idx', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('staged', [False, True])
def test_reference_run_scenes_per_bin(make_engine, golden_dir, idx, staged):
    """Five long scenes (201 frames, fixed consecutive seeds, incl. a 4 x 4 one) run through the reference's own offline_tango:
    disco_tango_enhance (fused and staged) per (node, bin) at 1e-4 on every bin under the fixture's sensitivity cut, the excluded
    share bounded, all bins at 1e-4 against the float64 restatement (tests/golden/make_golden_scenes.py)."""
    print(pc.check_reference_scene_per_bin(make_engine, golden_dir, idx, staged=staged))


@pytest.mark.parametrize('name,staged', [('c3', False), ('c3', True), ('c2', False)])
def test_baseline_shapes_vs_reference(make_engine, golden_dir, name, staged):
    """BASELINE.json's own shapes at full length (4 x 4 and 1 x 4, L = 160 000, 626 frames) run through the REFERENCE'S offline_tango
    (tests/golden/make_golden_baseline_shapes.py): fused and staged routes, whole signals at 1e-4 against the reference, every bin at
    2e-4, no bin excluded."""
    print(name, 'staged' if staged else 'fused', pc.check_baseline_shape_reference(make_engine, golden_dir, name, staged=staged))


def test_full_size_properties(make_engine):
    """Size-independent properties at the benchmark's per-room size, many rooms: (i) linearity of the filter stage
    -- apply(X, w) is linear in X; (ii) iSTFT(STFT(x)) == x; (iii) the MWF output is invariant to a common
    gain on the inputs (w^H y scales linearly, masks unchanged); (iv) batch independence: room r of a batch
    equals the same room processed alone."""
    pc.check_size_independent_properties(make_engine, R=6, K=4, M=4, L=160000)




def test_no_allocation_in_compute_calls(make_engine):
    print(pc.check_no_allocation_in_compute_calls(make_engine, K=4, M=4, L=20000))


@pytest.mark.parametrize('K,M,n_fft,L,tuning', [(2, 8, 512, 20000, None), (6, 4, 512, 20000, (0, 3, 0, 0)), (4, 8, 1024, 40000, None),
                                                (8, 8, 512, 30000, (0, 2, 0, 0)), (8, 4, 512, 20000, None), (8, 8, 1024, 40000, None),
                                                (2, 8, 512, 5120, (0, 20, 0, 0))])
def test_room_cov(make_engine, K, M, n_fft, L, tuning):
    """k_room_cov (csrc/k_room.h) against the staged route it replaces (DISCO_ROOM_COV=0) and against the float64 oracle."""
    print(pc.check_room_cov(make_engine, K=K, M=M, L=L, n_fft=n_fft, R=1 if K * M > 32 else 2, tuning=tuning))


@pytest.mark.parametrize('K,M,n_fft,L,pairs,R', [(8, 8, 1024, 40000, 0, 3), (8, 8, 1024, 24000, 2, 1), (2, 8, 1024, 30011, 0, 5), (6, 4, 512, 20000, 0, 2),
                                                 (4, 8, 512, 16384, 3, 2), (8, 4, 1024, 16384, 5, 2), (2, 8, 512, 300, 0, 2)])
def test_apply_istft_wide(make_engine, K, M, n_fft, L, pairs, R):
    """k_apply_istft_wide (csrc/k_fused.h: the wide shapes' final filter + iSTFT in one pass) against disco_apply + disco_istft (yf bit for
    bit, the samples to rounding) and against the float64 oracle: C5's shape, short runs (several chunks per node, runs past the end of
    the signal), a clip of one hop, lengths that are and are not multiples of the hop."""
    print(pc.check_apply_istft_wide(make_engine, K=K, M=M, L=L, n_fft=n_fft, R=R, pairs=pairs, oracle=L > 1000))


@pytest.mark.parametrize('mode', [2])
@pytest.mark.parametrize('K,M,n_fft,iters,R', [(4, 4, 512, 1, 5), (1, 4, 512, 1, 4), (8, 8, 1024, 2, 2), (2, 8, 512, 2, 3)])
def test_overlapped_halves(make_engine, K, M, n_fft, iters, R, mode):
    """disco_set_option("overlap_solves"): the whole-path calls as two half-batch children, the second on the context's side stream
    (fork / join with events): bit-identical to the plain call, two launches per stage, no allocation."""
    print(pc.check_overlapped_halves(make_engine, K=K, M=M, L=20000, n_fft=n_fft, R=R, iters=iters, mode=mode))


def test_reference_steps_state(make_engine):
    assert pc.check_reference_steps_state(make_engine, K=3, M=2, L=16000)


def test_engine_on_another_device():
    """Every entry point switches to the context's own device -- the plain memory helpers included (round-2 advice): an engine on
    device 1 while device 0 is current must allocate, copy and compute on device 1 and leave device 0 current.  On a box with ONE GPU
    there is no device 1: the engine must be refused with the device named -- never run on device 0 instead -- and device 0 stays current."""
    import torch
    from disco_amd import _lib
    from disco_amd.engine import DiscoError, Engine
    torch.cuda.set_device(0)
    if torch.cuda.device_count() < 2:
        with pytest.raises(DiscoError, match='no HIP device 1'):
            Engine(rooms=2, nodes=1, mics=3, length=4000, device=1, lib=_lib.load())
        assert torch.cuda.current_device() == 0
        return
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 4000)).astype(np.float32)
    ref = Engine(rooms=2, nodes=1, mics=3, length=4000, device=0, lib=_lib.load()).stft(x).numpy()
    eng = Engine(rooms=2, nodes=1, mics=3, length=4000, device=1, lib=_lib.load())
    X = eng.stft(x)                                    # DevBuf allocation + h2d + kernel + d2h, all on device 1
    assert torch.cuda.current_device() == 0
    assert np.array_equal(X.numpy(), ref)
    # and a caller-owned buffer ON device 1 is written by the same context while device 0 stays current
    t = torch.empty(ref.shape + (2,), dtype=torch.float32, device='cuda:1')
    eng._chk(eng.lib.disco_stft(eng.ctx, eng.to_device(x, np.float32)[0], 2, 3, t.data_ptr(), None))
    eng.sync()
    assert np.array_equal(torch.view_as_complex(t).cpu().numpy(), ref)


@pytest.mark.parametrize('K,M,L', [(4, 4, 40000), (2, 4, 16000), (8, 8, 64000)])     # (8 x 8: 1024-point frames; the sparsest statistic keeps 21 of its 126 frames, more than P = 15)
def test_saturating_masks_scored_against_the_reference_solve(make_engine, K, M, L):
    """Predicted masks that saturate whole bins (Rss ~ 0, Rnn ~ 0, both; one float32 rounding below 1): the unflagged bins at 1e-4 against
    the float64 oracle, every flagged (node, bin) within max(2 x the reference's own complex64 eig + clamp noise, 1e-4), output finite
    (round-5 VERDICT 'next' item 2; internal_formulas.py:56-73, tango.py:209-215, 387-394)."""
    print(pc.check_saturating_masks(make_engine, K=K, M=M, L=L, n_fft=512 if M < 8 else 1024))
