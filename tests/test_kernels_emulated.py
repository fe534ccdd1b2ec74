"""Kernel LOGIC under the hipemu CPU emulator (no GPU): the unmodified sources of disco_amd/csrc are compiled by
g++ against tests/hipemu and driven through the same C ABI / Engine as on the MI355X, at toy sizes, and
compared with the oracle.  This is test tooling, not a product path (disco_amd itself has no CPU path); the
real parity tests are tests/test_gpu_parity.py (-m gpu)."""
import numpy as np
import pytest

import emu_build
import parity_checks as pc
from disco_amd import synth
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_pk_operations(make_engine):
    pc.check_pk_selftest(make_engine, n=512)


def test_emu_room_primitives(make_engine):
    print(pc.check_room_selftest(make_engine, n=1024))


def test_emu_dpp_operations(make_engine):
    print(pc.check_dpp_selftest(make_engine, n=256))


@pytest.mark.parametrize('n_fft,L,chans', [(512, 1500, 3), (512, 2048, 2), (1024, 2600, 1), (512, 9000, 4), (1024, 2600, 3), (1024, 9000, 8),
                                           (512, 2000, 5), (512, 4500, 8), (1024, 2100, 4)])
@pytest.mark.parametrize('pad_mode', ['reflect', 'constant'])
def test_emu_stft(make_engine, n_fft, L, chans, pad_mode):
    print(pc.check_stft(make_engine, n_sig=2, chans=chans, L=L, n_fft=n_fft, pad_mode=pad_mode))


@pytest.mark.parametrize('n_fft,L', [(512, 2048), (512, 2100), (1024, 4500)])
def test_emu_istft(make_engine, n_fft, L):
    print(pc.check_istft(make_engine, n_sig=2, L=L, n_fft=n_fft))


def test_emu_masks(make_engine):
    print(pc.check_masks(make_engine, L=1800))
    print(pc.check_masks(make_engine, L=5000))


@pytest.mark.parametrize('K,M,same_z,mask_remote', [(2, 2, True, True), (3, 2, False, False), (1, 4, True, True)])
def test_emu_cov_solve_apply(make_engine, K, M, same_z, mask_remote):
    print(pc.check_cov_solve_apply(make_engine, R=1, K=K, M=M, L=2304, same_z=same_z, mask_remote=mask_remote))


@pytest.mark.parametrize('K,M,L,n_fft', [(1, 4, 23000, 512), (2, 3, 6000, 512), (1, 2, 9000, 1024)])
def test_emu_stft_cov_fused(make_engine, K, M, L, n_fft):
    print(pc.check_stft_cov_fused(make_engine, R=1, K=K, M=M, L=L, n_fft=n_fft))


@pytest.mark.parametrize('K,M', [(4, 4), (2, 2), (3, 2), (1, 3)])
def test_emu_step2_fused(make_engine, K, M):
    print(pc.check_step2_fused(make_engine, R=1, K=K, M=M, L=2304))


def test_emu_step2_reuse(make_engine):
    print(pc.check_step2_reuse(make_engine, R=1, K=3, M=2, L=2304))


def test_emu_online_golden(make_engine, golden_dir):
    print(pc.check_online_golden(make_engine, golden_dir, t_max=5))


def test_emu_online_stream(make_engine):
    """The streaming form of the online path == the whole-clip call, bit for bit, for several chunkings.  With the default options both
    shapes (P <= 7) run the thread kernel; the group kernel's streams are in tests/test_online_sizes_emulated.py."""
    print(pc.check_online_stream(make_engine, R=1, K=2, M=2, L=3072, update_every=3))
    print(pc.check_online_stream(make_engine, R=1, K=4, M=4, L=2048, update_every=2, chunks=(3, 1, 2)))


def test_emu_online_mwf(make_engine):
    print(pc.check_online_mwf(make_engine, R=1, K=2, M=2, L=1280, update_every=3))


def test_emu_metrics(make_engine, golden_dir):
    print(pc.check_metrics(make_engine, golden_dir, L_cut=1500, start=200))


def test_emu_ivad(make_engine, golden_dir):
    print(pc.check_ivad(make_engine, golden_dir))


@pytest.mark.parametrize('Ld,Lh,out_len', [(1500, 300, None), (1100, 1030, 2600)])
def test_emu_rir_convolve(make_engine, Ld, Lh, out_len):
    print(pc.check_rir_convolve(make_engine, n_sig=2, n_ch=2, Ld=Ld, Lh=Lh, out_len=out_len))


def test_emu_iterated(make_engine):
    print(pc.check_iterated(make_engine, K=2, M=1, L=1792, iters=2))


def test_emu_crnn_features():
    import emu_build
    print(pc.check_crnn_features(emu_build.load_emu(), 'cpu'))


def test_emu_conv3x3_pool4():
    import emu_build
    print(pc.check_conv3x3_pool4(emu_build.load_emu(), 'cpu'))


def test_emu_gru_gates():
    print(pc.check_gru_gates(emu_build.load_emu(), 'cpu'))


def test_emu_maxpool_last4():
    print(pc.check_maxpool_last4(emu_build.load_emu(), 'cpu'))


def test_emu_crnn_windows():
    print(pc.check_crnn_windows(emu_build.load_emu(), 'cpu'))


def test_emu_ism_pinned(make_engine):
    print(pc.check_ism_pinned_hip(make_engine))


def test_emu_ism_rir(make_engine):
    print(pc.check_ism_rir(make_engine, n_room=1, S=1, Q=2, max_order=3, rir_len=1024))


def test_emu_solver_singular_noise(make_engine):
    print(pc.check_solver_singular_noise(make_engine))


def test_emu_node_sharded(make_engine):
    print(pc.check_node_sharded(make_engine, R=1, K=2, M=2, L=4096, world=2))


def test_emu_solver_vs_reference_golden(make_engine, golden_dir):
    print(pc.check_solver_vs_reference_golden(make_engine, golden_dir))


@pytest.mark.parametrize('staged', [False, True])
def test_emu_tango_end_to_end(make_engine, staged):
    y, s, n = synth.make_rooms_numpy(1, K=2, M=2, L=8192)
    print(pc.check_tango_end_to_end(make_engine, y, s, n, staged_step2=staged))


def test_emu_solver_sizes(make_engine):
    print(pc.check_solver_sizes(make_engine, sizes=(1, 2, 3, 4, 5, 7, 8, 9, 15, 16), n=40))


def test_emu_solver_small_gap(make_engine):
    print(pc.check_solver_small_gap(make_engine, sizes=(2, 4, 7, 15)))


def test_emu_solver_routes(make_engine):
    print(pc.check_solver_routes(make_engine))


def test_emu_solver_routes_thread_vs_group(make_engine):
    """5 <= P <= 8: one thread per pencil (default) against the LDS group solver (option "solve_thread" 0), full matrices and -- through the
    partial sums of a covariance call -- both loaders (round-4 ADVICE: the non-default route had no test)."""
    print(pc.check_solver_routes(make_engine, sizes=(5, 6, 7, 8), n=21, option='solve_thread'))
    for M in (5, 7):
        for thread in (0, 1):
            print(M, thread, pc.check_cov_solve_apply(make_engine, R=1, K=1, M=M, L=12800, options={'solve_thread': thread}))


def test_emu_solver_degenerate(make_engine):
    pc.check_solver_degenerate(make_engine)


@pytest.mark.parametrize('sizes,option,value', [((1, 2, 3, 4), None, None), ((5, 7, 8), 'solve_thread', 1), ((5, 7, 8), 'solve_thread', 0),
                                                ((9, 12, 15, 16), 'solve_dpp', 1), ((9, 12, 15, 16), 'solve_dpp', 0)])
def test_emu_solver_indefinite(make_engine, sizes, option, value):
    """Indefinite pencils: the top eigenpair, on every route (the plain-statement forms of csrc/k_solve*.h)."""
    print(pc.check_solver_indefinite(make_engine, sizes=sizes, option=option, value=value, per_case=3))


def test_emu_mwf_variants(make_engine):
    print(pc.check_mwf_variants(make_engine, sizes=(1, 2, 3, 4, 5, 8, 9, 15, 16), n=9))


@pytest.mark.parametrize('K,M,L,n_fft,tuning', [(2, 2, 25700, 512, (80, 1, 1, 64)), (3, 2, 13000, 512, (13, 2, 3, 5)),
                                               (2, 2, 9000, 512, (80, 1, 1, 2)), (2, 1, 20000, 1024, (7, 1, 2, 0)),
                                               (1, 3, 25700, 512, (80, 1, 1, 64)), (1, 4, 9000, 512, (9, 1, 1, 4)), (1, 2, 5000, 1024, (3, 1, 1, 2)),
                                               (4, 4, 5000, 512, None), (2, 3, 9000, 512, (80, 1, 1, 3)), (3, 2, 2304, 512, (5, 2, 2, 2)), (2, 1, 700, 512, None)])
def test_emu_tango_pinned_geometry(make_engine, K, M, L, n_fft, tuning):
    """Large-batch launch geometries (long STFT runs with short / empty last waves, single-chunk covariances, many frame
    pairs per filter+iSTFT workgroup) pinned on a small batch through disco_set_tuning."""
    y, s, n = synth.make_rooms_numpy(2, K=K, M=M, L=L)
    print(pc.check_tango_end_to_end(make_engine, y, s, n, n_fft=n_fft, tol=1e-4, tuning=tuning))


@pytest.mark.parametrize('idx,staged', [(3, False), (3, True), (1, False)])
def test_emu_reference_run_scenes_per_bin(make_engine, golden_dir, idx, staged):
    """The kernel sources on the long reference-run scenes, per (node, bin) (tests/golden/make_golden_scenes.py)."""
    print(pc.check_reference_scene_per_bin(make_engine, golden_dir, idx, staged=staged))


def test_emu_no_allocation_in_compute_calls(make_engine):
    print(pc.check_no_allocation_in_compute_calls(make_engine))


@pytest.mark.parametrize('mode', [2])
@pytest.mark.parametrize('K,M,n_fft,iters,R', [(2, 2, 512, 1, 3), (1, 3, 512, 1, 2), (2, 8, 512, 2, 2), (3, 2, 1024, 2, 3)])
def test_emu_overlapped_halves(make_engine, K, M, n_fft, iters, R, mode):
    """disco_set_option("overlap_solves"): two half-batch children on two streams, bit-identical to the plain call."""
    print(pc.check_overlapped_halves(make_engine, K=K, M=M, L=3000 if n_fft == 512 else 5000, n_fft=n_fft, R=R, iters=iters, mode=mode))


def test_emu_reference_steps_state(make_engine):
    assert pc.check_reference_steps_state(make_engine)
