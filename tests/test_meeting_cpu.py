"""The reference side of tests/meeting_checks.py alone (no GPU, no emulator): the conditions under which its comparisons mean something.
  - C_MEETING is 4 x the worst err / (delta G) of the float32 NumPy restatement over the committed cases, and the restatement's mix
    spectrum lies inside C_MEETING delta with the same factor to spare;
  - the band in which an 'ibm' decision is not held holds at most 0.1 % of a case's bins;
  - the cases cover what the issue names: both FFT sizes and paddings, one pair, a lone last source, several pairs, the run edges, wave
    counts that leave empty waves in the last workgroup;
  - the NumPy statement of the mixes is what its docstring says (and sums in the stated order, which differs from other orders);
  - sir_valid / get_value_range restate the reference's functions (tests/golden/meeting_ref.npz) -- these need no device at all;
  - the C ABI and the package declare the new surface, and the package does not import matplotlib."""
import os
import subprocess
import sys

import numpy as np
import pytest

import meeting_checks as mk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_is_declared():
    from disco_amd import _lib, dataset_utils
    from disco_amd.engine import Engine
    hdr = open(os.path.join(REPO, 'include', 'disco_hip.h')).read()
    for name in ('disco_source_mix', 'disco_source_masks'):
        assert name in _lib.PROTOTYPES and f'int {name}(' in hdr, name
    assert len(_lib.PROTOTYPES['disco_source_mix'][1]) == 12 and len(_lib.PROTOTYPES['disco_source_masks'][1]) == 7
    assert all(callable(getattr(dataset_utils, f)) and f in dataset_utils.__all__
               for f in ('simulate_meetings', 'sir_at_nodes', 'sir_valid', 'get_value_range', 'meeting_rooms', 'meeting_masks'))
    assert callable(Engine.source_mix) and callable(Engine.source_masks)
    k_stft, k_room = (open(os.path.join(REPO, 'disco_amd', 'csrc', f)).read() for f in ('k_stft.h', 'k_roomsynth.h'))
    assert 'void k_source_masks(' in k_stft and 'void k_source_mix(' in k_room


def test_the_package_does_not_import_matplotlib():
    code = 'import sys; import disco_amd.dataset_utils; sys.exit(int(any(m.split(".")[0] == "matplotlib" for m in sys.modules)))'
    assert subprocess.run([sys.executable, '-B', '-c', code], cwd=REPO).returncode == 0


def test_mask_constant_is_four_times_the_float32_restatement():
    worst = mk.f32_restatement_ratio()
    per_s = {S: round(max(mk.mask_case(*c)['kinds'][k]['f32_ratio'] for c in mk.mask_cases() if c[2] == S for k in mk.VALUE_KINDS), 4) for S in mk.MASK_S}
    mix = max(mk.mask_case(*c)['mix_f32_ratio'] for c in mk.mask_cases())
    print('meeting masks: float32 restatement worst err / (delta G)', round(worst, 4), 'per S', per_s, 'C', mk.C_MEETING, '; mix worst err / delta', round(mix, 4))
    assert mk.C_MEETING == pytest.approx(4 * worst, rel=2e-3)
    assert mix <= mk.C_MEETING, "the restatement's own mix spectrum lies inside the bar the issue sets for it"


def test_ibm_band_holds_at_most_1e3_of_the_bins():
    frac = mk.ibm_band_fraction()
    zero = sum(int(mk.mask_case(*c)['kinds']['ibm1']['zero'].sum()) for c in mk.mask_cases())
    print('meeting ibm band fraction', frac, '; bins of exactly zero noise, held to the float32 decision:', zero)
    assert frac <= 1e-3
    assert zero > 0, 'a case with S = 2 has frames in which the other source is silent'


def test_cases_hold_the_promised_shapes():
    cases = mk.mask_cases()
    assert {c[:2] for c in cases} == {(n, p) for n in (512, 1024) for p in ('reflect', 'constant')}
    for key in {c[:2] for c in cases}:
        mine = [c for c in cases if c[:2] == key]
        assert sorted(c[2] for c in mine) == list(mk.MASK_S) and sorted(c[3] for c in mine) == list(mk.MASK_T), key
    assert len({(c[2], c[3]) for c in cases}) == len(cases), 'every setting pairs S and T differently'
    for n_fft, pad, S, T, L, n_sig in cases:
        assert T == 1 + L // (n_fft // 2) and L % (n_fft // 2)
        assert (n_sig * -(-T // 16)) % 4, 'the last workgroup has empty waves'
    cut = mk.mask_cases(cut=True)
    assert set(cut) <= set(cases) and {c[:2] for c in cut} == {c[:2] for c in cases} and any(c[3] > 16 for c in cut)
    for c in cases:
        img = mk.mask_case(*c)['img']
        assert not img[0, 0, :c[4] // 3].any() and img[0, 0, c[4] // 3:].all() and img[1:].all()
        rms = np.sqrt(np.mean(img[:, -1].astype(np.float64) ** 2, axis=1))
        assert 25 < rms.max() / rms.min() < 40, 'levels spread over 1.5 decades'


def test_mix_reference_sums_in_the_stated_order():
    img = np.zeros((3, 1, 2, 4), np.float32)
    img[:, 0, 0] = [[1, 2, 3, 4], [10, 20, 30, 40], [100, 200, 300, 400]]
    img[:, 0, 1] = [[2 ** 24, -0.0, 1, 5], [1, -0.0, 2 ** 24, 5], [1, -0.0, -2 ** 24, 5]]
    y, s, n = mk.mix_reference(img, np.array([1, 2]), stop=np.array([[4, 3]]))
    assert y[0, 0].tolist() == [111, 222, 333, 444] and s[0, 0].tolist() == [10, 20, 30, 40] and n[0, 0].tolist() == [101, 202, 303, 404]
    # (2^24 + 1) + 1 = 2^24 in float32, 1 + (1 + 2^24) likewise: the order shows in the third sample, (1 + 2^24) - 2^24 = 0 but 1 + (2^24 - 2^24) = 1
    assert y[0, 1].tolist() == [2 ** 24, 0, 0, 0] and np.signbit(y[0, 1, 1]) and not np.signbit(y[0, 1, 3])
    assert s[0, 1].tolist() == [1, 0, -2 ** 24, 0] and n[0, 1].tolist() == [2 ** 24, 0, 2 ** 24, 0] and np.signbit(n[0, 1, 1])
    img2, target = mk.mix_scene(8, 64, 1)
    y, _, n = mk.mix_reference(img2, target)
    other = img2[::-1].sum(axis=0, dtype=np.float32)
    assert np.mean(y != other) > 0.2, 'another order of the same additions gives other bits'
    assert set(target.tolist()) >= {0, 7}


def test_sir_valid_and_value_range_restate_the_reference():
    mk.check_sir_valid_golden()
    fx = mk.fixture()
    names = [k[6:] for k in fx if k.startswith('valid_')]
    assert all(fx[f'valid_{n}'].any() and not fx[f'valid_{n}'].all() for n in names), 'every sequence has both verdicts'
    for n in ('fill_n4', 'fill_n9'):                                         # a class that fills: accepted rooms, then refusals inside the same class
        v, s0 = fx[f'valid_{n}'], fx[f'sirs_{n}'][:, 0]
        inside = (s0 > 5) & (s0 < 8)
        level = int(np.ceil(int(fx[f'args_{n}'][0]) / 4))
        assert v[inside].sum() == level + 1 and (~v[inside]).sum() >= 2, (n, v, 'the strict comparison admits level + 1 rooms')
    v = fx['valid_rules_S2']
    assert v.tolist() == [False, False, True, True, False, False, True, True, False, True, False]
    v, s = fx['valid_first_only'], fx['sirs_first_only']
    assert v[(s[:, 0] > 8)].sum() >= 2, 'the second source crowds the class 2-5 / 8-11 without filling it for the first'
