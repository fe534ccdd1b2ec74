"""Checks of the context family: a context and the two half-batch children of its overlapped whole-path calls (option "overlap_solves",
csrc/host.h: for_family, child_follow, reserve_family).  Whatever per-context state a setter changes -- the tuning, an option that
changes the route, the per-room lengths, the stage timers -- the children must follow, whether they exist when the setter is called or
are created after it.  Shared by tests/test_gpu_context_family.py (MI355X, `-m gpu`) and tests/test_context_family_emulated.py (hipemu);
`make_engine(**cfg)` builds a disco_amd.engine.Engine bound to the library under test.

The yardstick is the plain call: an engine with overlap_solves = 0 and the same settings.  Rooms are independent and the children keep
the launch geometry of the whole batch, so the overlapped call's outputs equal the plain call's BIT FOR BIT
(parity_checks.check_overlapped_halves holds that for the bare case; here under every setter).  A characterisation of the host layer:
the device bytes the family owns after every step of a sequence are returned, and the emulated test pins them."""
import functools

import numpy as np

HOP = 256
# the smallest shapes at which the family can go wrong: halves of 1 and 2 rooms (every child offset non-zero, the halves differ); halves
# of 1 and 1; one wide shape (P2 = 9) that takes the room pass and the wide filter + iSTFT, through disco_tango_enhance_iterated
SHAPES = {
    'fused-R3': dict(R=3, K=2, M=2, L=15 * HOP, iters=0, options=('packed_x',)),
    'fused-R2': dict(R=2, K=2, M=2, L=15 * HOP, iters=0, options=('packed_x',)),
    'wide-R3': dict(R=3, K=2, M=8, L=23 * HOP, iters=1, options=('room_cov', 'fuse_wide_istft')),
}
TUNING = (2, 3, 2, 4)                    # frames per wave, covariance chunks, step-2 chunks, iSTFT pairs: none the heuristic's choice
ORDERS = ('before', 'after')             # the setter before the children exist (then overlap_solves = 2), or after


def setters_of(shape):
    return ('tuning',) + SHAPES[shape]['options'] + ('lengths', 'stage_timing')


def cases():
    return [(shape, setter, order) for shape in SHAPES for setter in setters_of(shape) for order in ORDERS]


def lengths_of(shape):
    """[full, about 0.6 full, about 0.4 full], all above n_fft / 2 + 1"""
    L = SHAPES[shape]['L']
    return [L, int(0.6 * L) + 6, int(0.4 * L) + 4][:SHAPES[shape]['R']]


@functools.lru_cache(maxsize=None)
def _scene(shape):
    """-> y (R, K, M, L) and the oracle mask of the uniform batch's geometry, computed ONCE per shape (read only)"""
    from disco_amd import synth
    from oracle import mwf_oracle as mo
    from oracle import stft_oracle as so
    c = SHAPES[shape]
    y, s, n = synth.make_rooms_numpy(c['R'], K=c['K'], M=c['M'], L=c['L'])
    S = so.stft(s[:, :, 0].reshape(-1, c['L']), 512, HOP, 'reflect', np.complex128)
    N = so.stft(n[:, :, 0].reshape(-1, c['L']), 512, HOP, 'reflect', np.complex128)
    m = np.transpose(mo.tf_mask(S, N, type='irm1'), (0, 2, 1)).astype(np.float32)
    m = np.ascontiguousarray(m.reshape(c['R'], c['K'], m.shape[1], m.shape[2]))
    y.setflags(write=False)
    m.setflags(write=False)
    return y, m


def _apply(eng, shape, setter):
    if setter == 'tuning':
        eng.set_tuning(*TUNING)
    elif setter == 'lengths':
        eng.set_lengths(lengths_of(shape))
    elif setter == 'stage_timing':
        eng.stage_timing(True)
    else:
        eng.set_option(setter, 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    assert set(got) == set(want), (what, set(got), set(want))
    for key in want:
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (what, key)


def check_setter(make_engine, shape, setter, order):
    """-> the bytes the overlapped engine's family owns after: creation, each of the two steps (setter and overlap_solves = 2, in
    `order`), reserve(1).  Asserts what the module docstring says, for one setter."""
    c = SHAPES[shape]
    R, iters = c['R'], c['iters']
    y, m = _scene(shape)

    def engine():
        return make_engine(rooms=R, nodes=c['K'], mics=c['M'], length=c['L'], n_fft=512)

    def run(e):
        if iters:
            out, yf = e.tango_enhance_iterated(y, m, iters=iters)
            return dict(out=out.numpy(), yf=yf.numpy())
        out, z, yf = e.tango_enhance(y, m)
        return dict(out=out.numpy(), z=z.numpy(), yf=yf.numpy())

    def run_enhanced_only(e):
        return {} if iters else dict(out=e.tango_enhance(y, m, want_z=False, want_yf=False)[0].numpy())

    plain, over = engine(), engine()
    try:
        assert (plain.T, plain.F) == m.shape[2:]
        plain.set_option('overlap_solves', 0)
        _apply(plain, shape, setter)
        owned = [over.owned_bytes()]
        steps = [lambda: _apply(over, shape, setter), lambda: over.set_option('overlap_solves', 2)]
        for step in (steps if order == 'before' else steps[::-1]):
            step()
            owned.append(over.owned_bytes())
        over.reserve(1)
        owned.append(over.owned_bytes())
        if setter != 'stage_timing':                                       # (else it is on already: the children must have followed)
            plain.stage_timing(True)
            over.stage_timing(True)
        want, got = run(plain), run(over)
        rp, ro = plain.stage_report(), over.stage_report()
        plain.stage_timing(False)
        over.stage_timing(False)
        assert np.isfinite(want['out']).all() and want['out'].any()
        _same(got, want, 'overlapped call')
        assert set(ro) == set(rp) and rp, (set(rp), set(ro))
        for nm in rp:
            assert rp[nm][1:] == (1, R) and ro[nm][1:] == (2, R), (nm, rp[nm], ro[nm])
        want_enh = run_enhanced_only(plain)
        _same(run_enhanced_only(over), want_enh, 'overlapped call, enhanced output only')
        assert not plain.stage_report() and not over.stage_report(), 'the timers are off again, in the children too'
        assert over.owned_bytes() == owned[-1], 'a whole-path call allocated'
        if setter == 'lengths':
            for r, L in enumerate(lengths_of(shape)):
                assert not want['out'][r, :, L:].any() and want['out'][r, :, :L].any(), r
            # the children's slices do not leak into a plain call on the same engine
            over.set_option('overlap_solves', 0)
            _same(run(over), want, 'plain call on the engine with children')
            # ... and set_lengths(None) reaches the children: the uniform batch again, overlapped and plain
            plain.set_lengths(None)
            over.set_lengths(None)
            uniform = run(plain)
            assert uniform['out'][-1, :, lengths_of(shape)[-1]:].any()
            _same(run(over), uniform, 'plain call on the engine with children, lengths cleared')
            over.set_option('overlap_solves', 2)
            _same(run(over), uniform, 'overlapped call, lengths cleared')
            _same(run_enhanced_only(over), run_enhanced_only(plain), 'overlapped call, lengths cleared, enhanced output only')
            assert over.owned_bytes() == owned[-1], 'a whole-path call allocated'
        return tuple(owned)
    finally:
        plain.close()
        over.close()
