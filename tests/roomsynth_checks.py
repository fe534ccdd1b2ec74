"""Checks of the steps between a reverberated source and a room the path can enhance: the per-sample VAD (csrc/k_roomsynth.h
k_vad_samples), the scaled mix (k_mix_scaled), and the Python surface built on them (disco_amd.sigproc_utils.vad_oracle_batch /
increase_to_snr, disco_amd.dataset_utils.snr_at_mics / simulate_rooms / mix_rooms).

Shared by tests/test_gpu_roomsynth.py (real MI355X, `-m gpu`), tests/test_roomsynth_emulated.py (the same kernel sources under the hipemu
CPU emulator) and tests/test_roomsynth_cpu.py (the reference side alone: the conditions on the inputs).  `make_engine(**cfg)` builds a
disco_amd.engine.Engine bound to the library under test; the checks of the package-level functions use the package's own engine (the
emulated tier binds it to the emulator).

References and bars, none taken from a kernel's output:
  VAD       sample-exact against the reference's own vad_oracle_batch (tests/golden/ivad_ref.npz, roomsynth_ref.npz: produced by
            tests/golden/make_golden_*.py) and against `vad_restatement`, the NumPy statement of the kernel's arithmetic.  Sample-exact is
            meaningful only where no sample sits on the threshold: tests/test_roomsynth_cpu.py holds min |x2 - thr_| / thr_ >= 1e-4 on the
            reference side for every signal compared with the reference (`vad_margin`).
  mix       bit equality with np.float32(g) * n and s + that in float32.
  gains     max |out - ref| / max |ref| <= 3e-5: the project's bar for its level metrics against the reference is 2e-4 dB
            (parity_checks.check_metrics); a gain is 10^(dB / 20), so that bar is ln(10) / 20 * 2e-4 = 2.3e-5 relative, plus one float32
            rounding of the product (6e-8) -- 3e-5.  Fed back into fw_snr: snr_out within 4e-4 dB, two applications of the same bar.
  SNRs      snrs and nodes_snr within 2e-4 dB of the reference's snr_at_mics, min_abs_delta (a difference of two) within 4e-4 dB.
  rooms     every piece of simulate_rooms bit-identical to the same public calls made by hand from the returned RIRs on (Engine.ism_rir sums
            with float atomics: its bits differ from call to call, so the RIRs are held to the float64 oracle at the existing 5e-6 of
            parity_checks.check_ism_rir); the images within the existing 2e-6 of np.convolve on the returned RIRs (check_rir_convolve).
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WINDOW_EDGES = (0, 1, 256, 257, 511, 512, 513, 768, 769)          # 512 / 256: 0 windows up to 256, 1 up to 512, 2 up to 768, 3 at 769
WINDOW_COUNTS = (0, 0, 0, 1, 1, 1, 2, 2, 3)
VAD_SETTINGS = ((256, 256, 2), (512, 512, 2), (1024, 256, 2), (512, 256, 1), (512, 256, 4))
GAIN_TOL, SNR_TOL = 3e-5, 2e-4
CASES = {'u': (2, 2), 'r': (2, 1), 't': (1, 1, 2)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = _bits(a) != _bits(b)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}'


def _small_engine(make_engine):
    return make_engine(rooms=1, nodes=1, mics=1, length=1024)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, 'roomsynth_ref.npz')))


@functools.lru_cache(maxsize=None)
def ivad_signals():
    """The three signals of tests/golden/ivad_ref.npz (L = 6000, 5121, 4096) with the reference's VAD of each."""
    z = np.load(os.path.join(GOLDEN, 'ivad_ref.npz'))
    return tuple((z[f'vad_x{i}'], z[f'vad_o{i}']) for i in range(int(z['n_vad'])))


# ---- the reference side ------------------------------------------------------------------------------------------------------------------
def n_windows(L, win_len=512, win_hop=256):
    """int(ceil((L - win_len) / win_hop + 1)), 0 when that is not positive, in integers."""
    a = L - win_len + win_hop
    return 0 if a <= 0 else -(-a // win_hop)


def vad_margin(x, thr=0.001):
    """min |x2 - thr_| / thr_ in the reference's own arithmetic (sigproc_utils.py:42-45) on the float32 signal."""
    d = x - np.mean(x)
    x2 = abs(d ** 2)
    thr_ = thr * np.quantile(x2, 0.99)
    return float(np.min(np.abs(x2 - thr_)) / thr_)


def vad_restatement(x, win_len=512, win_hop=256, thr=0.001, rat=2):
    """NumPy statement of k_vad_samples for one float32 signal: float64 mean rounded to float32, float32 squares, the two order statistics
    around (L - 1) q with q = float32(0.99), a float32 threshold, the integer window count."""
    x = np.asarray(x, np.float32)
    L = x.size
    vad = np.zeros(L, np.float32)
    if L == 0:
        return vad
    mean = np.float32(np.sum(x.astype(np.float64)) / L)
    d = x - mean
    x2 = np.abs(d * d)
    assert x2.dtype == np.float32
    vidx = (L - 1) * float(np.float32(0.99))
    k = int(vidx)
    srt = np.sort(x2)
    v_lo, v_hi = float(srt[k]), float(srt[min(k + 1, L - 1)])
    thr_ = np.float32(thr) * np.float32(v_lo + (v_hi - v_lo) * (vidx - k))
    over = x2 > thr_
    for w in range(n_windows(L, win_len, win_hop)):
        lo, hi = w * win_hop, min(w * win_hop + win_len, L)
        if over[lo:hi].sum() >= (hi - lo) // rat:
            vad[lo:hi] = 1
    return vad


def edge_signal(L=769, seed=5):
    """A constant plus bursts: the first burst lies inside the shortest clip that has a window (257 samples)."""
    rng = np.random.default_rng(seed)
    x = np.full(L, 0.05)
    for lo, hi in ((60, 200), (300, 420), (560, 700)):
        x[lo:min(hi, L)] += 0.3 * rng.standard_normal(max(min(hi, L) - lo, 0))
    return x.astype(np.float32)


def bursty(n_sig, L, seed):
    rng = np.random.default_rng(seed)
    x = 0.2 * rng.standard_normal((n_sig, L))
    gate = np.repeat(rng.random((n_sig, -(-L // 300))) < 0.55, 300, axis=1)[:, :L]
    return (x * gate + 0.01 * rng.standard_normal((n_sig, 1))).astype(np.float32)


def fma_case(n=4096, seed=31):
    """g, n, s (float32) on which a fused multiply-add gives another sum than s + fl(g n): s = -fl(g n) + j ulp, so that the sum with the
    rounded product is the exact small number j ulp, while the fused form also sees the rounding error of the product.  y - s == fl(g n)
    holds exactly for the unfused sum.  -> g, n, s, the unfused y, the fused y."""
    rng = np.random.default_rng(seed)
    g = np.float32(0.7310586)
    nn = rng.standard_normal(n).astype(np.float32)
    p = g * nn
    assert p.dtype == np.float32
    ulp = np.spacing(np.abs(p))
    s = (-p + rng.integers(1, 64, n).astype(np.float32) * ulp).astype(np.float32)
    y = s + p
    fused = (np.float64(g) * nn.astype(np.float64) + s.astype(np.float64)).astype(np.float32)      # g n and the sum are exact in float64
    return g, nn, s, y, fused


def mix_reference(s, n, gain, group, stop, L):
    """disco_mix_scaled in NumPy float32: n (n_sig, Ln), s (n_sig, L) or None -> n_out, y_out (n_sig, L)."""
    n_sig, Ln = n.shape
    n_out, y_out = np.zeros((n_sig, L), np.float32), np.zeros((n_sig, L), np.float32)
    for i in range(n_sig):
        Li = L if stop is None else int(stop[i])
        m = min(Ln, Li)
        n_out[i, :m] = np.float32(gain[i // group]) * n[i, :m]
        if s is not None:
            y_out[i, :Li] = s[i, :Li] + n_out[i, :Li]
    return n_out, y_out


def delta_all_pairs(nodes_snr):
    K = nodes_snr.shape[-1]
    return np.min([np.abs(nodes_snr[..., i] - nodes_snr[..., j]) for i in range(K) for j in range(i + 1, K)], axis=0)


def delta_consecutive(nodes_snr):
    """The reference's rule (convolve_signals.py:208-211): nodes_snr[i] - nodes_snr[i + 1] only."""
    return np.min(np.abs(nodes_snr[..., :-1] - nodes_snr[..., 1:]), axis=-1)


# ---- VAD ---------------------------------------------------------------------------------------------------------------------------------
def check_vad_golden(make_engine):
    """Sample-exact against the reference on the ivad_ref signals and on the target images of the fixture."""
    eng = _small_engine(make_engine)
    for i, (x, ref) in enumerate(ivad_signals()):
        got = eng.vad_samples(x)
        assert got.dtype == np.float32 and got.shape == x.shape
        bad = got != ref
        assert not bad.any(), f'ivad_ref signal {i} (L = {x.size}): {int(bad.sum())} samples wrong, first at {int(np.argmax(bad))}'
    fx = fixture()
    got = eng.vad_samples(fx['tar'])
    bad = got != fx['image_vad']
    assert not bad.any(), f'target images: {int(bad.sum())} samples wrong, first at {tuple(np.argwhere(bad)[0])}'
    assert np.all((got == 0) | (got == 1))


def check_vad_window_edges(make_engine):
    """L at every change of the window count at 512 / 256, sliced and through a stop per signal (L = 0 only so)."""
    eng = _small_engine(make_engine)
    x = edge_signal()
    rows = np.tile(x, (len(WINDOW_EDGES), 1))
    for i, L in enumerate(WINDOW_EDGES):
        rows[i, L:] = np.nan
    batch = eng.vad_samples(rows, stop=np.array(WINDOW_EDGES))
    for i, (L, nw) in enumerate(zip(WINDOW_EDGES, WINDOW_COUNTS)):
        assert n_windows(L) == nw, (L, n_windows(L), nw)
        want = vad_restatement(x[:L])
        if nw == 0:
            assert not want.any()
        _same_bits(batch[i, :L], want, f'L = {L} through stop')
        assert not batch[i, L:].any(), f'L = {L}: non-zero beyond stop'
        if L:
            _same_bits(eng.vad_samples(x[:L]), want, f'L = {L} sliced')


def check_vad_settings(make_engine, L=3001):
    eng = _small_engine(make_engine)
    x = bursty(2, L, 6)
    for win_len, win_hop, rat in VAD_SETTINGS:
        got = eng.vad_samples(x, win_len=win_len, win_hop=win_hop, rat=rat)
        for i in range(len(x)):
            _same_bits(got[i], vad_restatement(x[i], win_len, win_hop, rat=rat), f'{win_len}/{win_hop}, rat {rat}, signal {i}')
    assert 0 < eng.vad_samples(x[0]).mean() < 1, 'the input exercises both decisions'


def check_vad_stops(make_engine, L=3000, stops=(3000, 0, 1, 777, 2049, 513)):
    """A stop per signal: every row bit-identical to that row sliced and run alone, NaN at and beyond stop, zeros there in the output."""
    eng = _small_engine(make_engine)
    x = bursty(len(stops), L, 7)
    for i, st in enumerate(stops):
        x[i, st:] = np.nan
    got = eng.vad_samples(x, stop=np.array(stops))
    assert np.all((got == 0) | (got == 1))
    for i, st in enumerate(stops):
        assert not got[i, st:].any(), (i, st)
        if st:
            _same_bits(got[i, :st], eng.vad_samples(x[i, :st]), f'row {i} (stop {st}) against the row sliced and alone')
    two = eng.vad_samples(x.reshape(2, 3, L), stop=np.array(stops).reshape(2, 3))               # leading axes are a batch
    _same_bits(two.reshape(len(stops), L), got, 'a (2, 3, L) batch')
    x0 = bursty(2, L, 10)
    _same_bits(eng.vad_samples(x0, stop=700), np.concatenate([eng.vad_samples(x0[:, :700]), np.zeros((2, L - 700), np.float32)], axis=1), 'a scalar stop')


def check_vad_nan_isolation(make_engine, L=2500):
    eng = _small_engine(make_engine)
    x = bursty(3, L, 8)
    clean = eng.vad_samples(x)
    x[1, 1234] = np.nan
    got = eng.vad_samples(x)
    _same_bits(got[0], clean[0], 'row 0 beside a NaN row')
    _same_bits(got[2], clean[2], 'row 2 beside a NaN row')


def check_vad_against_ivad(make_engine, hop=256):
    """Two kernels, one decision: vad[t hop] == the 'ivad' mask at frame t for t < ceil(L / hop), on an engine of that length."""
    for i, (x, _) in enumerate(ivad_signals()):
        L = x.size
        eng = make_engine(rooms=1, nodes=1, mics=1, length=L, lazy_scratch=True)
        mask = eng.mask_ivad(x[None]).numpy()[0]
        vad = eng.vad_samples(x)
        n_t = -(-L // hop)
        _same_bits(np.ascontiguousarray(mask[:n_t, 0]), np.ascontiguousarray(vad[::hop][:n_t]), f'ivad_ref signal {i}')


def check_vad_refusals(make_engine):
    """The refusals leave vad untouched (a sentinel fill), through the C ABI itself."""
    from disco_amd import _lib
    eng = _small_engine(make_engine)
    L = 1024
    px, kx = eng.to_device(bursty(1, L, 9), np.float32)
    sentinel = np.full((1, L), -7.0, np.float32)
    pv, kv = eng.to_device(sentinel, np.float32)
    call = lambda length=L, win_len=512, win_hop=256, thr=0.001, rat=2, x=px, vad=pv: eng.lib.disco_vad_samples(
        eng.ctx, x, 1, length, None, win_len, win_hop, thr, rat, vad, eng.stream)
    for kw in (dict(win_len=500), dict(win_len=0), dict(win_hop=0), dict(rat=0), dict(thr=float('nan')), dict(thr=-1.0), dict(thr=float('inf')),
               dict(x=None), dict(vad=None)):
        assert call(**kw) == _lib.E_ARG, kw
    assert call(length=4096 * 256 + 1) == _lib.E_UNSUPPORTED
    assert b'4096' in eng.lib.disco_last_error(eng.ctx)
    assert eng.lib.disco_vad_samples(eng.ctx, px, -1, L, None, 512, 256, 0.001, 2, pv, eng.stream) == _lib.E_ARG
    eng.sync()
    _same_bits(kv.numpy(), sentinel, 'vad after the refusals')
    assert call() == 0                                                       # ... and the same buffers are then taken
    assert np.all(np.isin(kv.numpy(), (0.0, 1.0)))


# ---- mix ---------------------------------------------------------------------------------------------------------------------------------
def _mix_inputs(n_sig, L, Ln, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_sig, L)).astype(np.float32), rng.standard_normal((n_sig, Ln)).astype(np.float32), \
        (10.0 ** rng.uniform(-1, 1, n_sig)).astype(np.float32)


def check_mix_bits(make_engine, L=8192):
    """group 1 and 4, a shorter noise, the 16-byte and the scalar route, each output alone, a stop per signal with NaN beyond it."""
    eng = _small_engine(make_engine)
    for j, (n_sig, Lc, Ln, group, stops) in enumerate(((8, L, L, 1, False), (8, L, L, 4, False), (8, L, 5000, 4, False), (4, L, 5001, 1, False),
                                                       (4, L - 1, L - 1, 2, False), (8, L, 6000, 4, True), (3, 1027, 1027, 1, True), (2, 4, 4, 1, False))):
        s, n, g = _mix_inputs(n_sig, Lc, Ln, 40 + j)
        g = g[:n_sig // group]
        stop = None
        if stops:
            stop = np.random.default_rng(j).integers(0, Lc + 1, n_sig)
            stop[0], stop[-1] = Lc, 0
            for i, st in enumerate(stop):
                s[i, st:] = np.nan
                n[i, min(st, Ln):] = np.nan
        rn, ry = mix_reference(s, n, g, group, stop, Lc)
        what = f'n_sig {n_sig}, L {Lc}, Ln {Ln}, group {group}, stops {stops}'
        gn, gy = eng.mix_scaled(s, n, g, group=group, stop=stop)
        _same_bits(gn, rn, what + ': n_out')
        _same_bits(gy, ry, what + ': y_out')
        _same_bits(eng.mix_scaled(s, n, g, group=group, stop=stop, want_n=False)[1], ry, what + ': y_out alone')
        stop_n = None if stop is None else np.minimum(stop, Ln)              # without s the rows are Ln long
        only_n = eng.mix_scaled(None, n, g, group=group, stop=stop_n)
        assert only_n[1] is None
        _same_bits(only_n[0], mix_reference(None, n, g, group, stop_n, Ln)[0], what + ': n_out alone')


def check_mix_alignment_and_in_place(make_engine, n_sig=4, L=2048):
    """Rows offset by one float from 16-byte alignment (the scalar route on a length that would vectorise), and n_out == n in place."""
    eng = _small_engine(make_engine)
    s, n, g = _mix_inputs(n_sig, L, L, 50)
    rn, ry = mix_reference(s, n, g, 1, None, L)
    pad = lambda a: np.concatenate([np.zeros(1, np.float32), a.reshape(-1)])
    for off_s, off_n, off_o in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        sd = eng.to_device(pad(s), np.float32)[1].part(off_s, (n_sig, L)) if off_s else eng.to_device(s, np.float32)[1]
        nd = eng.to_device(pad(n), np.float32)[1].part(off_n, (n_sig, L)) if off_n else eng.to_device(n, np.float32)[1]
        no, yo = (eng.empty((n_sig * L + 1,), np.float32).part(off_o, (n_sig, L)) for _ in range(2))
        gn, gy = eng.mix_scaled(sd, nd, g, n_out=no, y_out=yo)
        assert gn is no and gy is yo
        _same_bits(no.numpy(), rn, f'offsets {off_s, off_n, off_o}: n_out')
        _same_bits(yo.numpy(), ry, f'offsets {off_s, off_n, off_o}: y_out')
    for off in (0, 1):                                                        # in place, both routes
        nd = eng.to_device(pad(n), np.float32)[1].part(off, (n_sig, L)) if off else eng.to_device(n, np.float32)[1]
        gn, gy = eng.mix_scaled(s, nd, g, n_out=nd)
        assert gn is nd
        _same_bits(nd.numpy(), rn, f'in place, offset {off}: n_out')
        _same_bits(gy.numpy(), ry, f'in place, offset {off}: y_out')


def check_mix_many_rows(make_engine, n_sig=70000, L=8):
    """More (row, chunk) items than the grid holds: the grid-stride loop."""
    eng = _small_engine(make_engine)
    s, n, g = _mix_inputs(n_sig, L, L, 51)
    rn, ry = mix_reference(s, n, g[:n_sig // 4], 4, None, L)
    gn, gy = eng.mix_scaled(s, n, g[:n_sig // 4], group=4)
    _same_bits(gn, rn, 'many rows: n_out')
    _same_bits(gy, ry, 'many rows: y_out')


def check_mix_no_fma(make_engine):
    """y_out - s == n_out bit for bit where a fused multiply-add would give another y (tests/test_roomsynth_cpu.py holds that it would)."""
    eng = _small_engine(make_engine)
    g, n, s, y, fused = fma_case()
    for want_n in (True, False):                                             # the product has one reader or two
        gn, gy = eng.mix_scaled(s[None], n[None], g, want_n=want_n)
        _same_bits(gy[0], y, f'y_out (want_n {want_n})')
        _same_bits(gy[0] - s, g * n, f'y_out - s (want_n {want_n})')
        if want_n:
            _same_bits(gn[0], g * n, 'n_out')


def check_mix_refusals(make_engine):
    from disco_amd import _lib
    eng = _small_engine(make_engine)
    s, n, g = _mix_inputs(4, 64, 64, 52)
    (ps, ks), (pn, kn), (pg, kg) = (eng.to_device(a, np.float32) for a in (s, n, g))
    out = eng.empty((4, 64), np.float32)
    call = lambda s_=ps, n_=pn, n_sig=4, L=64, Ln=64, g_=pg, group=1, no=out.ptr, yo=None: eng.lib.disco_mix_scaled(
        eng.ctx, s_ if yo else None, n_, n_sig, L, Ln, g_, group, None, no, yo, eng.stream)
    assert call() == 0
    for kw in (dict(no=None), dict(n_=None), dict(g_=None), dict(group=3), dict(group=0), dict(Ln=65), dict(n_sig=-1), dict(no=pn, Ln=32)):
        assert call(**kw) == _lib.E_ARG, kw
    assert eng.lib.disco_mix_scaled(eng.ctx, ps, pn, 4, 64, 64, pg, 1, None, out.ptr, None, eng.stream) == _lib.E_ARG      # s without y_out
    assert eng.lib.disco_mix_scaled(eng.ctx, None, pn, 4, 64, 64, pg, 1, None, None, out.ptr, eng.stream) == _lib.E_ARG    # y_out without s
    for bad, text in ((lambda: eng.mix_scaled(s, n[:3], g), 'leading axes'), (lambda: eng.mix_scaled(s[:, :32], n, g), 'longer'),
                      (lambda: eng.mix_scaled(s, n, g[:3]), 'gain'), (lambda: eng.mix_scaled(s, n, g, stop=np.arange(3)), 'broadcast'),
                      (lambda: eng.mix_scaled(s, n, g, stop=65), 'stop'), (lambda: eng.mix_scaled(s, n, g[:1], group=3), 'group')):
        try:
            bad()
        except ValueError as e:
            assert text in str(e), (text, str(e))
        else:
            raise AssertionError(f'not refused: {text}')


# ---- gains and SNRs (the package's own engine) ----------------------------------------------------------------------------------------------
def _vads(fx, with_vads):
    return (fx['vad_a'].astype(np.float32), fx['vad_b'].astype(np.float32)) if with_vads else (None, None)


def check_increase_to_snr():
    """Both weight settings, with and without VADs, against the reference's scaled noise (kept at every `sub`-th sample).  -> the figures."""
    from disco_amd import sigproc_utils as su
    fx = fixture()
    x, n, sub = fx['tar'][:, 0], fx['noi'][:, 0], int(fx['sub'])
    out = {}
    for w in (0, 1):
        for v in (0, 1):
            va, vb = _vads(fx, v)
            got = su.increase_to_snr(x, n, fx['snr_out'], vad_tar=va, vad_noi=vb, weight=bool(w), fs=int(fx['fs']))
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == n.shape
            ref = fx[f'scaled_w{w}_v{v}'].astype(np.float64)
            out[f'w{w}_v{v}'] = float(np.max(np.abs(got[:, ::sub] - ref).max(1) / np.abs(ref).max(1)))
    print('roomsynth increase_to_snr, worst |out - ref| / max |ref|:', out)
    assert max(out.values()) <= GAIN_TOL, out
    return out


def check_increase_to_snr_feedback():
    """The weight=True output, fed back into metrics.fw_snr, returns snr_out.  -> the worst distance in dB."""
    from disco_amd import metrics as dm
    from disco_amd import sigproc_utils as su
    fx = fixture()
    x, n, fs = fx['tar'][:, 0], fx['noi'][:, 0], int(fx['fs'])
    worst = 0.0
    for v in (0, 1):
        va, vb = _vads(fx, v)
        n_, gain = su.increase_to_snr(x, n, fx['snr_out'], vad_tar=va, vad_noi=vb, weight=True, fs=fs, return_gain=True)
        _same_bits(n_, gain.astype(np.float32)[:, None] * n, 'the scaled noise is gain * n')
        back = dm.fw_snr(x, n_, fs, vad_tar=va, vad_noi=vb)[1]
        worst = max(worst, float(np.abs(back - fx['snr_out']).max()))
    print('roomsynth increase_to_snr fed back into fw_snr, worst |snr - snr_out| dB:', worst)
    assert worst <= 2 * SNR_TOL, worst
    return worst


def check_snr_at_mics():
    """Uniform, ragged and three-node mics_per_node, with vad_s and with vad_s + vad_n, against the reference's snr_at_mics."""
    from disco_amd.dataset_utils import snr_at_mics
    fx = fixture()
    fs = int(fx['fs'])
    out = {}
    for tag, mpn in CASES.items():
        nm = sum(mpn)
        s, n = np.ascontiguousarray(fx['tar'][:, :nm]), np.ascontiguousarray(fx['noi'][:, :nm])
        vs = np.ascontiguousarray(fx['image_vad'][:, :nm]).astype(np.float32)
        for vtag in ('s', 'sn'):
            vn = np.ascontiguousarray(np.broadcast_to(fx['vad_b'][:, None, :], s.shape)).astype(np.float32) if vtag == 'sn' else None
            snrs, nodes, delta = snr_at_mics(s, n, mpn, fs, vad_s=vs, vad_n=vn)
            assert snrs.shape == (3, nm) and nodes.shape == (3, len(mpn)) and delta.shape == (3,)
            e = (float(np.abs(snrs - fx[f'snrs_{tag}_{vtag}']).max()), float(np.abs(nodes - fx[f'nodes_{tag}_{vtag}']).max()),
                 float(np.abs(delta - fx[f'delta_{tag}_{vtag}']).max()))
            out[f'{tag}_{vtag}'] = e
            assert e[0] <= SNR_TOL and e[1] <= SNR_TOL and e[2] <= 2 * SNR_TOL, (tag, vtag, e)
            one = snr_at_mics(s[1], n[1], mpn, fs, vad_s=vs[1], vad_n=None if vn is None else vn[1])          # a single room: (n_mic, L)
            assert one[0].shape == (nm,) and one[2].shape == ()
            _same_bits(np.asarray(one[1]), nodes[1], 'one room alone')
    print('roomsynth snr_at_mics, worst |snrs|, |nodes_snr|, |min_abs_delta| distance in dB:', out)
    return out


# ---- rooms -------------------------------------------------------------------------------------------------------------------------------
def room_scene(R=3, n_mic=4, seed=60):
    rng = np.random.default_rng(seed)
    dims = np.array([[4.0, 5.0, 3.0], [5.5, 4.2, 2.8], [6.0, 3.5, 3.1]], np.float32)[:R]
    absorption = np.array([0.35, 0.5, 0.25], np.float32)[:R]
    src = (dims[:, None, :] * rng.uniform(0.2, 0.8, (R, 2, 3))).astype(np.float32)
    mic = (dims[:, None, :] * rng.uniform(0.15, 0.85, (R, n_mic, 3))).astype(np.float32)
    return dims, absorption, src, mic


ROOM_KW = dict(fs=16000, max_order=3, rir_len=512)


def _simulate(R, L, lo=-100.0, hi=100.0, min_delta=-1.0):
    from disco_amd.dataset_utils import simulate_rooms
    fx = fixture()
    dims, absorption, src, mic = room_scene(R)
    return simulate_rooms(fx['tar'][:R, 0, :L], fx['noi'][:R, 0, :L], dims, absorption, src, mic, (2, 2), 5.0, (lo, hi), min_delta, **ROOM_KW)


def check_simulate_rooms(R=3, L=8192):
    """Every returned piece bit-identical to the same public calls made by hand; the images within 2e-6 of np.convolve on the RIRs.
    The RIRs are the exception: k_ism_rir accumulates a response with float atomics in LDS, so two calls of Engine.ism_rir differ in the
    last bits (139 of 12 288 taps between two calls on the MI355X).  The returned RIRs are held to the float64 oracle at the existing
    5e-6 of the largest tap (parity_checks.check_ism_rir), and the by-hand sequence continues from them."""
    from disco_amd import sigproc_utils as su
    from disco_amd._engines import get_engine
    from disco_amd.dataset_utils import snr_at_mics
    fx = fixture()
    res = _simulate(R, L)
    dims, absorption, src, mic = room_scene(R)
    tar, noi = np.ascontiguousarray(fx['tar'][:R, 0, :L]), np.ascontiguousarray(fx['noi'][:R, 0, :L])
    eng = get_engine(rooms=1, nodes=1, mics=1, length=1024)
    tv = su.vad_oracle_batch(tar)
    noise, gain = su.increase_to_snr(tar, noi, 5.0, vad_tar=tv, weight=True, fs=16000, return_gain=True)
    got_img, got_rir = res['images'].numpy(), res['rirs'].numpy()
    assert got_img.shape == (2, R, 4, L) and got_rir.shape == (2, R, 4, 512)
    from oracle import ism_oracle as io
    e_rir = max(float(np.max(np.abs(got_rir[i, r, c] - (want := io.ism_rir(dims[r], float(absorption[r]), src[r, i], mic[r, c], 3, 16000.0, 343.0, 512)))) /
                      np.max(np.abs(want))) for i in range(2) for r in range(R) for c in range(4))
    print('roomsynth simulate_rooms, RIRs against the float64 oracle:', e_rir)
    assert e_rir < 5e-6, e_rir
    img_t = eng.rir_convolve(tar, got_rir[0], out_len=L).numpy()
    img_n = eng.rir_convolve(noise, got_rir[1], out_len=L).numpy()
    vad = su.vad_oracle_batch(img_t)
    snrs, nodes, diff = snr_at_mics(img_t, img_n, (2, 2), 16000, vad_s=vad)
    _same_bits(res['noise_dry'].numpy(), noise, 'noise_dry')
    _same_bits(res['noise_gain'], np.asarray(gain, np.float64), 'noise_gain')
    _same_bits(got_img[0], img_t, 'target images')
    _same_bits(got_img[1], img_n, 'noise images')
    _same_bits(res['image_vad'].numpy(), vad, 'image_vad')
    _same_bits(res['snr_images'], snrs, 'snr_images')
    _same_bits(res['snr_nodes'], nodes, 'snr_nodes')
    _same_bits(res['snr_diff'], diff, 'snr_diff')
    assert res['valid'].dtype == bool and res['valid'].all()
    assert 0 < vad.mean() < 1
    worst = 0.0
    for src_i, dry in ((0, tar), (1, noise)):
        for r in range(R):
            for c in range(4):
                want = np.convolve(dry[r].astype(np.float64), got_rir[src_i, r, c].astype(np.float64))[:L]
                worst = max(worst, float(np.max(np.abs(got_img[src_i, r, c] - want)) / np.max(np.abs(want))))
    print('roomsynth simulate_rooms, images against np.convolve:', worst)
    assert worst < 2e-6, worst
    return res


def valid_bounds(nodes, diff):
    """From the figures of a run: a setting under which every room is valid, and three under each of which exactly room `r` fails one
    condition alone; every bound at least 0.01 dB from every node SNR (and from every difference)."""
    flat = np.sort(nodes.reshape(-1))
    lo_all, hi_all, d_all = float(flat[0] - 1), float(flat[-1] + 1), float(diff.min() - 0.5)
    def between(values, above):                                              # a bound with exactly the smallest (largest) value on the wrong side
        v = np.sort(values)
        a, b = (v[0], v[1]) if above else (v[-2], v[-1])
        assert b - a >= 0.02, (a, b)
        return float((a + b) / 2)
    cases = [('all', (lo_all, hi_all, d_all), None),
             ('lo', (between(flat, True), hi_all, d_all), int(np.argmin(nodes.min(1)))),
             ('hi', (lo_all, between(flat, False), d_all), int(np.argmax(nodes.max(1)))),
             ('delta', (lo_all, hi_all, between(diff, True)), int(np.argmin(diff)))]
    for _, (lo, hi, d), _ in cases:
        assert np.abs(nodes - lo).min() >= 0.01 and np.abs(nodes - hi).min() >= 0.01 and np.abs(diff - d).min() >= 0.01
    return cases


def check_valid_flags(R=3, L=8192, base=None):
    base = base if base is not None else _simulate(R, L)
    for name, (lo, hi, d), bad_room in valid_bounds(base['snr_nodes'], base['snr_diff']):
        res = _simulate(R, L, lo, hi, d)
        want = np.ones(R, bool)
        if bad_room is not None:
            want[bad_room] = False
        assert np.array_equal(res['valid'], want), (name, res['valid'], want, res['snr_nodes'], res['snr_diff'])
        # a second run draws its RIRs again (float atomics: other last bits), so its figures move a little: well inside half the 0.01 dB
        # every bound keeps from every figure
        assert np.abs(res['snr_nodes'] - base['snr_nodes']).max() < 0.005 and np.abs(res['snr_diff'] - base['snr_diff']).max() < 0.005


def check_mix_rooms_tango(R=3, L=8192, lengths=(8192, 6000, 7000)):
    """mix_rooms -> offline_tango_batched on the device-resident outputs == the same call on their host copies; y == s + n exactly."""
    from disco_amd.dataset_utils import mix_rooms
    from disco_amd.engine import DevBuf
    from disco_amd.speech_enhancement.tango import offline_tango_batched
    fx = fixture()
    tar, noi = np.ascontiguousarray(fx['tar'][:R, :, :L]), np.ascontiguousarray(fx['noi'][:R, :, :L - 192])
    eng = _package_engine()
    tar_d = eng.to_device(tar, np.float32)[1]
    snr = np.array([5.0, 0.0, -3.0])[:R]
    lengths = np.array(lengths[:R], np.int32)
    y, s, n = mix_rooms(tar_d, noi, snr, (2, 2), lengths=lengths)
    assert all(isinstance(a, DevBuf) and a.shape == (R, 2, 2, L) for a in (y, s, n))
    assert s.ptr == tar_d.ptr, 's is a view of tar_img'
    yh, sh, nh = y.numpy(), s.numpy(), n.numpy()
    _same_bits(sh.reshape(tar.shape), tar, 's')
    for r in range(R):
        g = np.float32(10 ** (-snr[r] / 20))
        want_n = np.zeros((4, L), np.float32)
        m = min(int(lengths[r]), noi.shape[-1])
        want_n[:, :m] = g * noi[r, :, :m]
        _same_bits(nh[r].reshape(4, L), want_n, f'room {r}: n')
        want_y = np.zeros((4, L), np.float32)
        want_y[:, :lengths[r]] = (tar[r] + want_n)[:, :lengths[r]]
        _same_bits(yh[r].reshape(4, L), want_y, f'room {r}: y = s + n below its length, zeros beyond')
    dev = offline_tango_batched(y, s, n, lengths=lengths)
    host = offline_tango_batched(yh, sh, nh, lengths=lengths)
    assert set(dev) == set(host) and 'yf' in dev
    for k in dev:
        _same_bits(dev[k], host[k], f'offline_tango_batched[{k}] on the device-resident rooms')
    assert np.isfinite(dev['yf']).all() and np.abs(dev['yf']).max() > 0
    whole = mix_rooms(tar, fx['noi'][:R, :, :L], snr, (2, 2))                # NumPy in, no lengths: still on the device
    _same_bits(whole[0].numpy(), whole[1].numpy() + whole[2].numpy(), 'y == s + n')


def _package_engine():
    from disco_amd._engines import get_engine
    return get_engine(rooms=1, nodes=1, mics=1, length=1024)


def check_surface():
    """The container rule and the ValueErrors."""
    from disco_amd import sigproc_utils as su
    from disco_amd.dataset_utils import mix_rooms, snr_at_mics
    from disco_amd.engine import DevBuf
    eng = _package_engine()
    x = bursty(4, 1500, 70)
    v_host = su.vad_oracle_batch(x)
    assert isinstance(v_host, np.ndarray) and v_host.dtype == np.float32
    xd = eng.to_device(x, np.float32)[1]
    v_dev = su.vad_oracle_batch(xd)
    assert isinstance(v_dev, DevBuf) and v_dev.shape == x.shape
    _same_bits(v_dev.numpy(), v_host, 'device in, DevBuf out')
    _same_bits(su.vad_oracle_batch(x[0]), v_host[0], 'a single (L,) signal')
    assert su.vad_oracle_batch(x[0]).shape == (1500,)
    n_host = su.increase_to_snr(x, x[::-1].copy(), 3.0)
    n_dev = su.increase_to_snr(xd, eng.to_device(x[::-1].copy(), np.float32)[1], 3.0)
    assert isinstance(n_host, np.ndarray) and isinstance(n_dev, DevBuf)
    _same_bits(n_dev.numpy(), n_host, 'increase_to_snr: device in, DevBuf out')
    gn, gy = eng.mix_scaled(xd, xd, 0.5)
    assert isinstance(gn, DevBuf) and isinstance(gy, DevBuf)
    _same_bits(gy.numpy(), x + np.float32(0.5) * x, 'mix_scaled on DevBufs')

    def refused(fn, text):
        try:
            fn()
        except ValueError as e:
            assert text in str(e), (text, str(e))
        else:
            raise AssertionError(f'not refused: {text}')
    refused(lambda: su.vad_oracle_batch(x, stop=np.arange(3)), 'broadcast')
    refused(lambda: su.vad_oracle_batch(x, stop=1501), 'stop')
    refused(lambda: su.increase_to_snr(x, x, np.zeros(3)), 'broadcast')
    img = x.reshape(1, 4, 1500)
    refused(lambda: mix_rooms(img, img, 0.0, (3, 1)), '[3, 1]')
    refused(lambda: mix_rooms(img, img, [0.0, 1.0], (2, 2)), 'per room')
    refused(lambda: snr_at_mics(img, img, (2, 1)), 'add up')
    refused(lambda: snr_at_mics(img, img, (4,)), 'two nodes')
