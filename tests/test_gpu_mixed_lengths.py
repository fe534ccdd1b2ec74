"""Rooms of different clip lengths in one batch (disco_set_lengths, Engine.set_lengths, offline_tango_rooms) on a real MI355X: every
room of a mixed batch against the float64 oracle run on that room alone at its own length, on every route of the whole path
(tests/length_checks.py), and the whole path with lengths set captured into a hipGraph."""
import numpy as np
import pytest

import length_checks as lc
from disco_amd import _lib, synth
from disco_amd.engine import DiscoError, Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('chans', [1, 2, 4, 5, 8])
@pytest.mark.parametrize('pad_mode', ['reflect', 'constant'])
@pytest.mark.parametrize('n_fft', [512, 1024])
def test_stft_at_the_edges(make_engine, n_fft, pad_mode, chans):
    print(lc.check_stft_edges(make_engine, n_fft, pad_mode, chans))


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_istft_at_the_edges(make_engine, n_fft):
    print(lc.check_istft_edges(make_engine, n_fft))


@pytest.mark.parametrize('n_fft', [512, 1024])
def test_mask_oracle_at_the_edges(make_engine, n_fft):
    print(lc.check_mask_edges(make_engine, n_fft))


def test_cov_mean_over_own_frames(make_engine):
    assert lc.check_cov_mean(make_engine)


# lengths: every room keeps T_r >= 4 P2 + 4 frames and L_r % hop <= hop / 2 (tests/length_checks.py)
LENGTHS_K4M4 = (12288, 8193, 10000, 11100, 9216, 8320)                      # P2 = 7: T_r >= 32
LENGTHS_K8M8 = (40960, 33000, 36864, 34900)                                 # 1024 points, P2 = 15: T_r >= 64 frames of 512
LENGTHS_K16M2 = (20480, 18560, 19000, 18433)                                # P2 = 17: T_r >= 72


def test_whole_path_single_node(make_engine):
    lc.check_whole_path(make_engine, 1, 4, lc.LENGTHS_K3M2, want_stage='stft_apply_istft')


@pytest.mark.parametrize('staged', [False, True])
def test_whole_path_k3m2(make_engine, staged):
    lc.check_whole_path(make_engine, 3, 2, lc.LENGTHS_K3M2, staged_step2=staged, want_stage='cov2' if staged else 'step2_apply_istft')


def test_whole_path_k3m2_large_batch_geometry(make_engine):
    """the launch geometry a production batch takes: long frame runs, one chunk, long runs of frame pairs"""
    lc.check_whole_path(make_engine, 3, 2, lc.LENGTHS_K3M2, tuning=(40, 1, 1, 16), alone=False)


@pytest.mark.parametrize('overlap', [0, 2])
def test_whole_path_k4m4(make_engine, overlap):
    lc.check_whole_path(make_engine, 4, 4, LENGTHS_K4M4, overlap=overlap, want_stage='step2_apply_istft')


def test_whole_path_room_pass(make_engine):
    lc.check_whole_path(make_engine, 8, 8, LENGTHS_K8M8, n_fft=1024, want_stage='room_cov2')


def test_whole_path_room_pass_iterated(make_engine):
    lc.check_whole_path(make_engine, 8, 8, LENGTHS_K8M8, n_fft=1024, iters=2, want_stage='apply2_istft', alone=False)


def test_whole_path_room_pass_staged_tail(make_engine):
    lc.check_whole_path(make_engine, 8, 8, LENGTHS_K8M8[:2], n_fft=1024, options={'fuse_wide_istft': 0, 'room_cov': 0}, want_stage='istft',
                        alone=False)


def test_whole_path_wide(make_engine):
    lc.check_whole_path(make_engine, 16, 2, LENGTHS_K16M2, want_stage='cov2')


def test_alone_equals_batched_near_a_whole_hop(make_engine):
    lc.check_alone_equals_batched_near_whole_hop(make_engine)


def test_tango_reference_every_mode(make_engine):
    lc.check_reference_outputs(make_engine)


def test_uniform_batch_untouched(make_engine):
    assert lc.check_uniform_untouched(make_engine)


def test_refusals_and_arguments(make_engine):
    assert lc.check_refusals(make_engine, DiscoError)


def test_python_surface():
    lc.check_python_surface()


def test_no_allocation_with_lengths(make_engine):
    """after disco_reserve a call with lengths set allocates nothing; disco_set_lengths itself allocates its block once"""
    K, M, L, R = 3, 2, 8192, 3
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=L)
    eng.set_option('overlap_solves', 2)
    eng.reserve(2)
    eng.set_lengths([8192, 6272, 7000])
    own = eng.owned_bytes()
    m = eng.mask_oracle(s[:, :, 0].reshape(R * K, L), n[:, :, 0].reshape(R * K, L)).reshape(R, K, eng.T, eng.F)
    eng.tango_enhance(y, m)
    eng.tango_enhance(y, m, want_z=False, want_yf=False)
    eng.tango_enhance_iterated(y, m, iters=2)
    eng.tango_reference(y, s, n)
    eng.set_lengths([5120, 8192, 6000])
    eng.tango_enhance(y, m)
    assert eng.owned_bytes() == own


@pytest.mark.timeout(600)
@pytest.mark.parametrize('overlap', [0, 2])
def test_whole_path_with_lengths_replayed_from_a_hip_graph(overlap):
    """disco_mask_oracle + disco_tango_enhance captured with lengths set; replayed on fresh rooms, then with OTHER lengths set outside
    the capture (the kernels read them from the same device block): every replay equals the eager call with the same lengths bit for bit"""
    import torch
    lib = _lib.load()
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    R, K, M, L = 4, 4, 4, 24000
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=lib)
    eng.set_option('overlap_solves', overlap)
    eng.reserve(1)
    T, F, G = eng.T, eng.F, R * K
    y = torch.empty((R, K, M, L), dtype=torch.float32, device=dev)
    s_ref = torch.empty((R, K, L), dtype=torch.float32, device=dev)
    n_ref = torch.empty((R, K, L), dtype=torch.float32, device=dev)
    mask = torch.empty((R, K, T, F), dtype=torch.float32, device=dev)
    out = torch.empty((R, K, L), dtype=torch.float32, device=dev)

    def load(first_room):
        yh, sh, nh = synth.make_rooms_numpy(R, K=K, M=M, L=L, first_room=first_room)
        y.copy_(torch.from_numpy(yh))
        s_ref.copy_(torch.from_numpy(np.ascontiguousarray(sh[:, :, 0])))
        n_ref.copy_(torch.from_numpy(np.ascontiguousarray(nh[:, :, 0])))
        return yh, sh, nh

    def launch(stream):
        eng._chk(lib.disco_mask_oracle(eng.ctx, s_ref.data_ptr(), n_ref.data_ptr(), G, mask.data_ptr(), stream))
        eng._chk(lib.disco_tango_enhance(eng.ctx, y.data_ptr(), mask.data_ptr(), mask.data_ptr(), out.data_ptr(), None, None, None, 0, stream))

    first = [24000, 16640, 20000, 12400]
    other = [13000, 24000, 9216, 22100]
    eng.set_lengths(first)
    load(100)
    launch(None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch(side.cuda_stream)
    torch.cuda.synchronize()
    for first_room, lens in ((7, first), (31, first), (31, other), (7, other)):
        eng.set_lengths(lens)                              # outside the capture
        yh, sh, nh = load(first_room)
        out.fill_(-3.0)
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        out.fill_(-5.0)
        launch(None)
        torch.cuda.synchronize()
        eager = out.cpu().numpy()
        assert np.array_equal(got, eager), ('graph replay differs from the eager launch sequence', first_room, lens)
        from oracle import stft_oracle as so
        from oracle import tango_oracle as to
        for r, Lr in enumerate(lens):
            assert not got[r, :, Lr:].any()
        r = 3 if lens is first else 2                       # one short room against the oracle at its own length
        Lr = lens[r]
        o = to.offline_tango_vec(yh[r][..., :Lr], sh[r][..., :Lr], nh[r][..., :Lr], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
        for k in range(K):
            ref = so.istft(o['yf'][k], Lr, 512, 256, work_dtype=np.float64)
            assert lc.relerr(got[r, k, :Lr], ref) < 1e-4, (first_room, r, k)
