"""What a caller of the staged API can observe of the covariance partial sums a context holds between calls (csrc/host.h: the blocks the
covariance passes leave their unfinished sums in, the record of what is pending for disco_gevd_mwf_r1_pending, the record of the step-1
sums disco_step2_cov_fused_reuse pairs with), under the hipemu CPU emulator (no GPU): which configuration call drops what, the two
refusals of the re-use and the one of the pending solve by their messages, what the growth of a block under lazy_scratch forgets, that
owned_bytes() moves only where a block grew, and the pending solve after each of the five producers within the bars of
tests/cov_checks.py.  A characterisation: it states what the library does, so that a change of the host code that keeps this state
cannot move it unnoticed.  Test tooling only; the real runs are -m gpu.
Wall time: 36 s on an 8-core host run alone."""
import numpy as np
import pytest

import cov_checks as cc
import emu_build
import parity_checks as pc
from disco_amd.engine import DiscoError, Engine

M, K, T, N_FFT, F = 2, 3, 16, 512, 257
P2 = M + K - 1
NO_PENDING = 'no covariance call has left partial sums'
NO_STEP1 = 'no step-1 partial sums'
NOT_THE_ARRAYS = 'not the arrays'


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def _engine(make_engine, **kw):
    eng = make_engine(rooms=1, nodes=K, mics=M, length=(T - 1) * cc.HOP[N_FFT], n_fft=N_FFT, **kw)
    assert eng.T == T and eng.F == F
    return eng


def _refused(call, text):
    with pytest.raises(DiscoError) as e:
        call()
    assert 'error -1:' in str(e.value) and text in str(e.value), str(e.value)


def _bits(buf):
    return cc._bits(buf.numpy())


class Scene:
    """Exact spectra for the staged covariance calls and a clip for the fused step 1, each uploaded ONCE: the re-use is granted by the
    identity of the arrays, so the tests hold on to the device buffers."""

    def __init__(self, eng, seed=3):
        X, Zs, _zn, mask = cc.scene(seed, 1, K, M, T, F, True, solvable=True)
        self.X_h, self.Z_h, self.mask_h = X, Zs, mask
        self.X, self.Z, self.mask = (eng.to_device(a, d)[1] for a, d in ((X, np.complex64), (Zs, np.complex64), (mask, np.float32)))
        y, mask_y = cc.bursty_clip(np.random.default_rng(seed), K, M, eng.Lsamp, T, F, cc.HOP[N_FFT])
        self.y_h, self.mask_y_h = y, mask_y
        self.y, self.mask_y = eng.to_device(y, np.float32)[1], eng.to_device(mask_y, np.float32)[1]
        self.Xy = eng.empty((1, K, T, F, M), np.complex64)

    def step1_cov(self, eng):
        eng.cov_masked(self.X, self.mask, Rss_out=False)

    def step2_cov(self, eng):
        eng.cov_masked(self.X, self.mask, self.Z, self.Z, Rss_out=False)

    def step1_fused(self, eng):
        """-> w_loc: the fused STFT + covariance pass, its sums left pending, and their solve"""
        eng.stft_cov_fused(self.y, self.mask_y, X_out=self.Xy, want_cov=False)
        return eng.gevd_mwf_r1_pending(M)[0]

    def reuse(self, eng, w_loc, X=None, mask=None):
        return eng.step2_cov_fused_reuse(self.Xy if X is None else X, self.mask_y if mask is None else mask, w_loc, want_z=True)


@pytest.mark.parametrize('lazy', [False, True])
def test_fresh_engine_has_nothing_pending(make_engine, lazy):
    eng = _engine(make_engine, lazy_scratch=lazy)
    try:
        own = eng.owned_bytes()
        assert (own == 0) == lazy
        _refused(lambda: eng.gevd_mwf_r1_pending(M), NO_PENDING)
        sc = Scene(eng)
        _refused(lambda: sc.reuse(eng, eng.empty((1, K, F, M), np.complex64)), NO_STEP1)
        assert eng.owned_bytes() == own
    finally:
        eng.close()


def test_every_configuration_call_drops_the_pending_sums(make_engine):
    """set_tuning, set_node_shard (even to the shard in force) and set_lengths (to values, and back to None), each between a covariance
    call that leaves its sums pending and the solve: the solve refuses, the next covariance call is solved as before, nothing is allocated."""
    eng = _engine(make_engine)
    try:
        sc = Scene(eng)
        own = eng.owned_bytes()
        lens = [eng.Lsamp - 300]

        def solved(cov, P):
            cov(eng)
            return _bits(eng.gevd_mwf_r1_pending(P)[0])
        for cov, P in ((sc.step1_cov, M), (sc.step2_cov, P2)):
            first = solved(cov, P)
            assert np.array_equal(solved(cov, P), first)
            _bits_again = _bits(eng.gevd_mwf_r1_pending(P)[0])               # a solve does not consume the sums
            assert np.array_equal(_bits_again, first)
            for drop in (lambda: eng.set_tuning(0, 0, 0, 0), lambda: eng.set_tuning(cov_chunks=3), lambda: eng.set_tuning(0, 0, 0, 0),
                         lambda: eng.set_node_shard(0, K)):
                cov(eng)
                drop()
                _refused(lambda: eng.gevd_mwf_r1_pending(P), NO_PENDING)
            assert np.array_equal(solved(cov, P), first)
            cov(eng)
            eng.set_lengths(lens)
            _refused(lambda: eng.gevd_mwf_r1_pending(P), NO_PENDING)
            cov(eng)
            eng.gevd_mwf_r1_pending(P)
            eng.set_lengths(None)
            _refused(lambda: eng.gevd_mwf_r1_pending(P), NO_PENDING)
            assert np.array_equal(solved(cov, P), first)
        # options do not touch the sums
        sc.step1_cov(eng)
        w = _bits(eng.gevd_mwf_r1_pending(M)[0])
        sc.step1_cov(eng)
        eng.set_option('room_cov', 0)
        eng.set_z_blocks(1)
        eng.set_z_blocks(K)
        assert np.array_equal(_bits(eng.gevd_mwf_r1_pending(M)[0]), w)
        assert eng.owned_bytes() == own
    finally:
        eng.close()


def test_reuse_is_granted_for_the_arrays_of_step_1_only(make_engine):
    eng = _engine(make_engine)
    try:
        sc = Scene(eng)
        own = eng.owned_bytes()
        w_loc = sc.step1_fused(eng)
        z0 = _bits(sc.reuse(eng, w_loc))
        w0 = _bits(eng.gevd_mwf_r1_pending(P2)[0])
        # the step-1 sums stay: the re-use can be repeated, and a refusal changes nothing
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0) and np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)
        _refused(lambda: sc.reuse(eng, w_loc, mask=sc.mask_y_h), NOT_THE_ARRAYS)             # equal content, another array
        _refused(lambda: sc.reuse(eng, w_loc, X=sc.Xy.numpy()), NOT_THE_ARRAYS)
        _refused(lambda: sc.reuse(eng, w_loc, X=sc.X), NOT_THE_ARRAYS)
        assert np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)                     # the pending pencil is still the re-use's
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0) and np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)
        # what drops the step-1 sums
        for drop in (lambda: eng.set_tuning(0, 0, 0, 0), lambda: eng.set_lengths([eng.Lsamp]), lambda: eng.set_lengths(None),
                     lambda: sc.step2_cov(eng), lambda: eng.step2_cov_fused(sc.Xy, sc.mask_y, w_loc)):
            sc.step1_fused(eng)
            drop()
            _refused(lambda: sc.reuse(eng, w_loc), NO_STEP1)
            _refused(lambda: sc.reuse(eng, w_loc, mask=sc.mask_y_h), NO_STEP1)               # the first of the two refusals wins
        # what does not: the shard in force set again (it drops the PENDING sums only), options, the z layout
        assert np.array_equal(_bits(sc.step1_fused(eng)), _bits(w_loc))
        eng.set_node_shard(0, K)
        _refused(lambda: eng.gevd_mwf_r1_pending(M), NO_PENDING)
        eng.set_option('solve_thread', 1)
        eng.set_z_blocks(K)
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0) and np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)
        sc.reuse(eng, w_loc)
        eng.set_node_shard(0, K)
        _refused(lambda: eng.gevd_mwf_r1_pending(P2), NO_PENDING)
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0) and np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)
        # a real shard: the fused step 1 runs on it and keeps nothing for a re-use
        eng.set_node_shard(1, 2)
        eng.stft_cov_fused(sc.y_h[:, 1:], sc.mask_y_h[:, 1:], want_cov=False)
        eng.gevd_mwf_r1_pending(M)
        eng.set_node_shard(0, K)
        _refused(lambda: sc.reuse(eng, w_loc), NO_STEP1)
        # the staged step-1 covariance of the same arrays is a step 1 too
        eng.cov_masked(sc.Xy, sc.mask_y, Rss_out=False)
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0)
        assert np.isfinite(eng.gevd_mwf_r1_pending(P2)[0].numpy().view(np.float32)).all()
        assert eng.owned_bytes() == own
    finally:
        eng.close()


def test_a_grown_full_block_forgets_everything(make_engine):
    """lazy_scratch: the block of step 1 is too small for step 2.  A staged step 2 after it grows the block, gives the answer of an engine
    whose blocks were sized at creation bit for bit, and the step-1 sums are gone; reserve() growing the block between a covariance call
    and its solve leaves a refusal, not a solve of a fresh block."""
    ref, eng = _engine(make_engine), _engine(make_engine, lazy_scratch=True)
    try:
        sc_ref, sc = Scene(ref), Scene(eng)
        w_ref = sc_ref.step1_fused(ref)
        want_cov = [_bits(b) for b in ref.cov_masked(sc_ref.Xy, sc_ref.mask_y, sc_ref.Z, sc_ref.Z)]
        want_fused = [_bits(b) for b in ref.step2_cov_fused(sc_ref.Xy, sc_ref.mask_y, w_ref)]
        own_ref = ref.owned_bytes()
        for staged in (True, False):
            own = eng.owned_bytes()
            w_loc = sc.step1_fused(eng)
            assert np.array_equal(_bits(w_loc), _bits(w_ref))
            grown = eng.owned_bytes()
            assert grown > own or not staged                                 # the first pass allocates the block of step 1
            if staged:
                got = [_bits(b) for b in eng.cov_masked(sc.Xy, sc.mask_y, sc.Z, sc.Z)]
                assert all(np.array_equal(g, w) for g, w in zip(got, want_cov))
                assert eng.owned_bytes() > grown                             # ... and step 2 a larger one
            else:
                got = [_bits(b) for b in eng.step2_cov_fused(sc.Xy, sc.mask_y, w_loc)]
                assert all(np.array_equal(g, w) for g, w in zip(got, want_fused))
                assert eng.owned_bytes() == grown                            # (second round: the block is large enough by now)
            _refused(lambda: sc.reuse(eng, w_loc), NO_STEP1)
        eng.close()
        eng = _engine(make_engine, lazy_scratch=True)
        sc = Scene(eng)
        w_loc = sc.step1_fused(eng)
        own = eng.owned_bytes()
        assert 0 < own < own_ref
        eng.reserve(0)
        assert eng.owned_bytes() == own_ref
        _refused(lambda: eng.gevd_mwf_r1_pending(M), NO_PENDING)
        _refused(lambda: sc.reuse(eng, w_loc), NO_STEP1)
        # with the blocks at full size the same sequence keeps both records
        assert np.array_equal(_bits(sc.step1_fused(eng)), _bits(w_ref))
        eng.reserve(0)
        assert np.array_equal(_bits(eng.gevd_mwf_r1_pending(M)[0]), _bits(w_ref))
        sc.reuse(eng, w_loc)
        assert eng.owned_bytes() == own_ref == ref.owned_bytes()
    finally:
        ref.close()
        eng.close()


def test_a_grown_tail_block_drops_only_the_pencil_pending_in_it(make_engine):
    """lazy_scratch with the step-2 geometry pinned below the staged one: the tail block a re-use allocates is smaller than what
    reserve() asks for while the full block already has that size.  reserve() then grows the tail block alone: the pencil pending in it
    is refused, the step-1 sums in the full block survive and the re-use is granted again, with the same answer."""
    eng = _engine(make_engine, lazy_scratch=True)
    try:
        sc = Scene(eng)
        eng.set_tuning(cov_chunks=8, step2_chunks=2)
        assert eng.owned_bytes() == 0
        sc.step2_cov(eng)                                                    # the full block at its largest
        full = eng.owned_bytes()
        assert full == K * 8 * F * (P2 * (P2 + 1) // 2) * 16
        w_loc = sc.step1_fused(eng)
        assert eng.owned_bytes() == full
        z0 = _bits(sc.reuse(eng, w_loc))
        assert eng.owned_bytes() == full + full // 4                         # the tail block: 2 chunks
        w0 = _bits(eng.gevd_mwf_r1_pending(P2)[0])
        sc.reuse(eng, w_loc)
        eng.reserve(0)
        assert eng.owned_bytes() == 2 * full
        _refused(lambda: eng.gevd_mwf_r1_pending(P2), NO_PENDING)
        assert np.array_equal(_bits(sc.reuse(eng, w_loc)), z0) and np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w0)
        # a pencil pending in the FULL block is not touched by the growth of the tail block
        eng.close()
        eng = _engine(make_engine, lazy_scratch=True)
        sc = Scene(eng)
        eng.set_tuning(cov_chunks=8, step2_chunks=2)
        sc.step2_cov(eng)
        w2 = _bits(eng.gevd_mwf_r1_pending(P2)[0])
        eng.reserve(0)
        assert eng.owned_bytes() == 2 * full
        assert np.array_equal(_bits(eng.gevd_mwf_r1_pending(P2)[0]), w2)
    finally:
        eng.close()


def test_pending_solve_after_each_producer(make_engine):
    """cov_partials (k_cov, k_cov_loc_f64's (hi, lo) pairs), cov_partials_wide and step2_cov_partials through check_pending,
    stft_cov_partials and the re-use's two blocks through check_reuse, room_cov_partials (and the staged route's own re-use, which only a
    whole-path call reaches) through check_room_cov: each within the bars those helpers hold."""
    print(cc.check_pending(make_engine, T_all=29, chunk_counts=(1, 3), families=('k_cov', 'k_cov_loc_f64', 'k_cov_wide', 'k_step2_cov_fused')))
    print(cc.check_reuse(make_engine, shapes=[(2, 3), (7, 2)], T=32))
    print(pc.check_room_cov(make_engine, K=2, M=8, L=3000, n_fft=512, R=1))
