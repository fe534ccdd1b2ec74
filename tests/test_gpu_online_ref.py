"""Scoring the online mode on a real MI355X (tests/online_ref_checks.py): the companion kernels of csrc/k_online_ref.h at every pencil
size and route, the whole path disco_tango_online_reference, and the Python surface on top of it.

Kernels launched here: k_online_mwf_thread_ref<1> .. <7> with packed-float32 and with float64 squarings; k_online_mwf_ref<5>, <6>, <7>
("solve_thread" = 0), k_online_mwf_ref<8> (8 lanes per problem) and k_online_mwf_ref<9> .. <16> (16 lanes per problem).  Lines starting
with "online_ref " carry what the GPU showed."""
import numpy as np
import pytest

import online_ref_checks as rc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def make_engine():
    lib = _lib.load()          # raises if the gfx950 library is missing: no fallback

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


@pytest.mark.parametrize('variant', ['d1', 'd1e-3'])
def test_every_size_and_route(make_engine, variant):
    """Checks 1 and 2: P = 1 .. 16 in the step-1 form, every step-2 shape, every route: out_s and out_n inside their bars, out and
    w_last equal to disco_online_mwf's."""
    print('online_ref_sizes_errors', variant, rc.check_sizes(make_engine, variant))


def test_filter_in_force(make_engine):
    """Check 3: update_every in {1, 2, 3, T - 1, T, T + 5}, companions compared frame by frame."""
    print(rc.check_schedule(make_engine))


def test_row_order_and_layouts(make_engine):
    """Check 4: K = 6 (P = 7, both routes) and K = 9 with M = 8 (P = 16): node shards at every k0, rank-major z blocks bit-identical."""
    print(rc.check_row_order(make_engine))


def test_one_companion(make_engine):
    """Check 5: n_comp = 1 gives the out_s of the two-companion call, bit for bit."""
    rc.check_one_companion(make_engine)


def test_companions_do_not_feed_the_recursion(make_engine):
    """Check 6: a NaN in S, then in one remote Zs row, stays in out_s at its own problems and frame."""
    rc.check_containment(make_engine)


def test_argument_refusals(make_engine):
    rc.check_refusals(make_engine)


@pytest.mark.parametrize('K,M,opts', [(3, 2, None), (4, 4, None), (4, 4, {'solve_thread': 0})])
def test_whole_path(make_engine, K, M, opts):
    """Check 8: check_online_mwf's rooms, and P2 = 7 on both routes."""
    rc.check_whole_path(make_engine, K=K, M=M, options=opts)


def test_surface():
    rc.check_surface()


def test_signals_go_through_batch_results():
    """Check 9, last part: the (6, R, K, L) signals, device resident, through results_io.batch_results -- the values of the same call on
    host copies of the same six signals, to the bit (the device-against-host requirement of span_checks.check_batch_results, which
    this mirrors: np.testing.assert_array_equal)."""
    import torch
    from disco_amd import synth
    from disco_amd.speech_enhancement import results_io as rio
    from disco_amd.speech_enhancement import tango
    R, K, M, L, fs = 2, 3, 2, 6000, 2000
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    yd, sd, nd = (torch.from_numpy(a).cuda() for a in (y, s, n))
    sig = torch.empty((6, R, K, L), dtype=torch.float32, device='cuda')
    d = tango.online_tango_batched(yd, sd, nd, signals=sig)
    assert d['signals'] is sig and d['yf'].shape == (R, K, 1 + L // 256, 257)
    torch.cuda.synchronize()
    snrs = np.zeros((R, K))
    ch0 = lambda a: a[:, :, 0].contiguous()
    dev = rio.batch_results(ch0(sd), ch0(nd), sig[1], sig[2], sig[4], sig[5], snrs, fs=fs, y_in=ch0(yd), sh_t=sig[0], szh_t=sig[3])
    h = sig.cpu().numpy()
    host = rio.batch_results(s[:, :, 0], n[:, :, 0], h[1], h[2], h[4], h[5], snrs, fs=fs, y_in=y[:, :, 0], sh_t=h[0], szh_t=h[3])
    for a, b in zip(dev, host):
        assert tuple(a) == tuple(b)
        for key in a:
            np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]), err_msg=key)
    print('online_ref scores: snr_out', np.asarray(dev[0]['snr_out']).round(2).tolist(), 'step 1', np.asarray(dev[1]['snr_out']).round(2).tolist())


def test_graph_capture(make_engine):
    """Check 10: after disco_reserve, disco_tango_online_reference captured on a stream and replayed gives the eager result bit for
    bit, and the library owns no more memory after the call than before it."""
    import ctypes as C
    import torch
    from disco_amd import _lib as L
    from disco_amd import synth
    R, K, M, Ls = 2, 3, 2, 6000
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=Ls)
    eng = make_engine(rooms=R, nodes=K, mics=M, length=Ls)
    eng.reserve(2)
    owned = eng.owned_bytes()
    yd, sd, nd = (torch.from_numpy(a).cuda() for a in (y, s, n))
    names = ('yf', 'sf', 'nf', 'z_y', 'z_s', 'z_n', 'zn', 'masks_z', 'mask_w')

    def outputs():
        spec = {nm: torch.zeros((R, K, eng.T, eng.F), dtype=torch.float32 if nm.startswith('mask') else torch.complex64, device='cuda')
                for nm in names}
        return spec, torch.zeros((6, R, K, Ls), dtype=torch.float32, device='cuda')

    def call(spec, sig, stream):
        outs = L.DiscoRefOutputs(**{nm: t.data_ptr() for nm, t in spec.items()})
        eng._chk(eng.lib.disco_tango_online_reference(eng.ctx, yd.data_ptr(), sd.data_ptr(), nd.data_ptr(), None, None, 0.95, 2, 1e-3,
                                                      C.byref(outs), sig.data_ptr(), None, 0, stream))
    eager, eager_sig = outputs()
    call(eager, eager_sig, None)
    torch.cuda.synchronize()
    assert eng.owned_bytes() == owned
    spec, sig = outputs()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(spec, sig, side.cuda_stream)
    torch.cuda.synchronize()
    assert float(sig.abs().max()) == 0.0                  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert eng.owned_bytes() == owned
    for nm in names:
        assert torch.equal(torch.view_as_real(spec[nm]) if spec[nm].is_complex() else spec[nm],
                           torch.view_as_real(eager[nm]) if eager[nm].is_complex() else eager[nm]), nm
    assert torch.equal(sig, eager_sig) and float(eager_sig.abs().max()) > 0
    eng.close()
