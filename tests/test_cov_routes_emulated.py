"""The masked-covariance kernels (csrc/k_cov.h, k_cov_wide.h, k_fused.h k_step2_cov_fused) under the hipemu CPU emulator (no GPU): the
exact tier of tests/test_gpu_cov_routes.py through the same C ABI and Engine, cut to one room and at most 5 frames (exactness does not
depend on the frame count) -- every kernel family, every M of k_cov and of k_step2_cov_fused, node shards, per-room lengths, NaN
containment, the refusals, one chunk of 66 frames for the stride of the Nyquist wave, and the pending solves of four families.
Test tooling only; the real runs are -m gpu.
Wall time: 110 s on an 8-core host run alone (about twice that inside a run of the whole CPU suite)."""
import pytest

import cov_checks as cc
import emu_build
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_cut_covers_every_family_and_mic_count():
    names = cc.launched_by(cc.exact_cases(cut=True))
    for fam in ('k_cov<', 'k_cov_loc_f64<7>', 'k_cov_loc_f64<8>', 'k_cov_split_lds<', 'k_cov_big<true>', 'k_cov_big<false>', 'k_cov_wide<true>',
                'k_cov_wide<false>', 'k_step2_cov_fused<'):
        assert any(n.startswith(fam) for n in names), fam
    for M in range(1, 9):
        assert any(n.startswith(f'k_step2_cov_fused<{M},') for n in names), M
    for M in range(1, 8):
        assert any(n.startswith(f'k_cov<{M},') and not n.startswith(f'k_cov<{M},0,') for n in names), M
    for M in range(1, 7):
        assert any(n.startswith(f'k_cov<{M},0,') for n in names), M


@pytest.mark.parametrize('T', [4, 5])
def test_emu_every_family_exact(make_engine, T):
    """T = 4: bit equality; T = 5: the two roundings of the mean."""
    cases = cc.exact_cases(cut=True)
    if T == 5:
        cases = [c for c in cases if c['K'] <= 16]
    print(cc.check_exact_cases(make_engine, cases, T=T))


def test_emu_launch_geometry(make_engine):
    print(cc.check_geometry(make_engine, cc.GEOMETRY_CUT, long_families=('k_cov',)))


def test_emu_node_shards_and_z_blocks(make_engine):
    print(cc.check_shards(make_engine, T=3, every_k0=False))


def test_emu_per_room_lengths(make_engine):
    print(cc.check_lengths(make_engine, T=5))


def test_emu_nan_stays_in_its_pencils(make_engine):
    cc.check_nonfinite(make_engine, T=5)


def test_emu_refusals_leave_the_context_usable(make_engine):
    cc.check_refusals(make_engine)


def test_emu_pending_solves_read_every_partial_block(make_engine):
    """All four loaders: k_solve_small.h (k_cov, k_cov_loc_f64, fused), k_solve.h (the /group entries), k_solve_dpp.h (k_cov_split_lds),
    k_solve_wide.h (k_cov_wide)."""
    print(cc.check_pending(make_engine, T_all=29, chunk_counts=(1, 3), families=('k_cov', 'k_cov_loc_f64', 'k_cov_loc_f64/group', 'k_cov_split_lds',
                                                                                 'k_cov_big/group', 'k_cov_wide', 'k_step2_cov_fused')))


def test_emu_reuse_route(make_engine):
    print(cc.check_reuse(make_engine, shapes=[(1, 2), (2, 3), (4, 4), (7, 2), (1, 8), (3, 6)], T=64))


def test_emu_float32_accumulation(make_engine):
    """96 frames in one chunk; the bar is measured on the spot (the committed table is for 626)."""
    print(cc.check_float(make_engine, families=('k_cov', 'k_cov_big', 'k_cov_split_lds'), T=96))


def test_emu_stft_cov_fused_against_the_float64_transform(make_engine):
    """The committed table's own cases (the shorter ones): both FFT sizes, the staged pair, empty waves, 2 and 3 frames, lengths."""
    print(cc.check_stft_cov(make_engine, ids=('512-M1', '512-M4', '512-M8', '1024-M3', '1024-M6', '1024-M7', 'empty-waves', 'T2', 'T3',
                                               'T3-1024', 'lengths-512', 'lengths-run40', 'lengths-staged')))
