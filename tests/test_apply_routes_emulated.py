"""The filter-and-sum and inverse-transform kernels (csrc/k_apply.h, k_fused.h k_step2_apply_fused / k_step2_apply_istft /
k_apply_istft_wide, k_stft.h k_istft) under the hipemu CPU emulator (no GPU): a cut of tests/test_gpu_apply_routes.py through the same C
ABI and Engine -- one room pair, at most 5 frames for the exact tier (exactness does not depend on the frame count; the launch-geometry tests alone run 17, 64 and 66 frames), every kernel
family and every M, node shards, per-room lengths, NaN containment, the refusals, and one run-boundary case per inverse-transform
kernel.  Test tooling only; the real runs are -m gpu.
Wall time: 15 s on an 8-core host."""
import pytest

import apply_checks as ac
import emu_build
from disco_amd.engine import Engine


@pytest.fixture(scope='module')
def make_engine():
    lib = emu_build.load_emu()

    def mk(**cfg):
        return Engine(lib=lib, **cfg)
    return mk


def test_emu_cut_covers_every_family_and_mic_count():
    names = ac.launched_by_exact(cut=True) | ac.launched_by_istft(cut=True)
    for fam in ('k_apply<', 'k_apply_m<', 'k_apply_mq<', 'k_step2_apply_fused<', 'k_step2_apply_istft<512,', 'k_apply_istft_wide<512,',
                'k_apply_istft_wide<1024,', 'k_istft<512,false>', 'k_istft<1024,false>'):
        assert any(n.startswith(fam) for n in names), fam
    for M in range(1, 9):
        assert any(n.startswith(f'k_apply<{M},0>') for n in names) and any(n.startswith(f'k_step2_apply_fused<{M},') for n in names), M
        assert f'k_apply_m<{M},31>' in names, M
    for M in range(1, 8):
        assert any(n.startswith(f'k_apply<{M},') and not n.endswith(',0>') for n in names), M
    for M in (1, 2, 3, 5, 6, 7):
        assert f'k_apply_m<{M},15>' in names, M
    assert {n for n in ac.reachable() if n.startswith('k_apply_mq')} <= names
    assert all(c['T'] <= 5 for c in ac.apply_cases(cut=True))


def test_emu_disco_apply_every_family_exact(make_engine):
    print(ac.check_apply_cases(make_engine, ac.apply_cases(cut=True)))


def test_emu_step2_apply_fused_exact(make_engine):
    for M, K in ac.FUSED_CUT:
        ac.check_step2_fused(make_engine, M, K, T=5 if M % 2 else 4)
    ac.check_step2_fused(make_engine, 2, 2, 1024, T=2)
    print(ac.check_geometry_fused(make_engine, geom=((1, 0), (2, 700), (5, 2), (5, 3), (66, 1))))


def test_emu_apply_istft_fused_spectra_exact(make_engine):
    for n_fft, M, K in ac.WIDE_CUT:
        ac.check_wide_yf(make_engine, n_fft, M, K, T=3 if n_fft == 512 else 2)


def test_emu_heads_and_residuals(make_engine):
    ac.check_heads_and_residuals(make_engine)


def test_emu_launch_geometry(make_engine):
    print(ac.check_geometry_apply(make_engine, geom={'k_apply_m': ((3, 8), (17,)), 'k_apply_mq': ((8, 4), (17,)), 'k_apply': ((2, 3), (64,))}))


def test_emu_node_shards_and_z_blocks(make_engine):
    print(ac.check_shards(make_engine, T=2, every_k0=False, wide=False))


def test_emu_per_room_lengths(make_engine):
    print(ac.check_lengths(make_engine, T=5))


def test_emu_nan_stays_where_the_algebra_puts_it(make_engine):
    ac.check_nonfinite(make_engine, T=3, shapes=((2, 3), (3, 8), (4, 6)))


def test_emu_refusals_leave_the_context_usable(make_engine):
    ac.check_refusals(make_engine)


def test_emu_inverse_transforms_per_hop_segment(make_engine):
    """One run-boundary case per kernel (n_seg = one run plus one segment), a short clip each, and the fused kernels against the staged calls."""
    for fam, v in ac.check_istft_cases(make_engine, ac.istft_cases(cut=True)).items():
        print('apply_routes_errors', fam, v)


def test_emu_nan_frame_stays_within_two_frames(make_engine):
    ac.check_istft_nonfinite(make_engine, n_seg=11, t0=5)
