"""What the level checks rest on, without a library or a GPU: the fixture of tests/golden/levels_ref.npz is what its generator makes and
covers the listed cases, the derived bars are what the checks modules state, the special reverberation rows do what they were built
for, ci_wp / bar_data equal the reference's values, and the new names exist where a user of the reference looks for them."""
import numpy as np

import reverb_checks as rc
import segsnr_checks as sg


def test_fixture_is_the_generators_and_small():
    g = sg.golden()
    assert all(isinstance(v, np.ndarray) for v in g.values())
    import os
    assert os.path.getsize(os.path.join(sg.HERE, 'golden', 'levels_ref.npz')) < 1 << 20
    for k in range(len(rc.gen.REVERB_SHAPES)):
        x, rir, rs, kinds, drr, srr = rc.golden_shape(k)
        Ld, Lh, n_sig, n_ch = rc.gen.REVERB_SHAPES[k]
        assert x.shape == (n_sig, Ld) and rir.shape == (n_sig, n_ch, Lh) and x.dtype == rir.dtype == np.float32
        assert np.all(np.isfinite(drr)) and np.all(np.isfinite(srr))


def test_seg_snr_cases_cover_the_list():
    cases = sg.gen.seg_cases()
    for w, h in sg.gen.SEG_WINDOWS:
        lens = {int(c[2] - c[1]) for c in cases if (c[3], c[4]) == (w, h)}
        assert {w - 1, w, w + h - 1, w + h, 6000} <= lens, (w, h, lens)
    assert {int(c[5]) for c in cases} == {sg.gen.VAD_NONE, sg.gen.VAD_BINARY, sg.gen.VAD_FRACTION, sg.gen.VAD_ZERO}
    assert any(c[1] == 300 for c in cases)
    s, n, vad = sg.gen.seg_signals()
    assert np.all(s[1, 512:1280] == 0) and np.all(n[1, 2048:2816] == 0) and np.all(s[1, 3584:4352] == 0) and np.all(n[1, 3584:4352] == 0)
    assert abs(s[2, 1000:2100].mean()) > 900 and set(np.unique(vad[0])) == {0.0, 1.0} and np.all(vad[2] == 0) and 0 < vad[1].min() < vad[1].max() < 1
    ref = sg.golden()['seg_ref']
    assert np.nanmin(ref) >= -15 and np.nanmax(ref) <= 25


def test_seg_snr_yardstick_restated():
    """The definition of the issue restated in a few lines of float64 NumPy equals the reference's values: the fixture pins the definition
    the kernel documents (whole windows only, vad[start + m hop] as the weight)."""
    g = sg.golden()
    worst = 0.0
    eps = np.finfo(np.float64).eps
    for (row, start, stop, w, h, v), want in zip(g['seg_cases'], g['seg_ref']):
        a, b = g['seg_s'][row, start:stop].astype(np.float64), g['seg_n'][row, start:stop].astype(np.float64)
        n_w = (len(a) - w) // h + 1 if len(a) >= w else 0
        if n_w == 0:
            assert np.isnan(want)
            continue
        win = lambda x: np.stack([x[m * h:m * h + w] for m in range(n_w)])
        val = np.clip(10 * np.log10(np.maximum(win(a).var(axis=1), eps) / np.maximum(win(b).var(axis=1), eps)), -15, 25)
        wt = np.ones(n_w) if v == sg.gen.VAD_NONE else g['seg_vad'][v, start:stop:h][:n_w].astype(np.float64)
        with np.errstate(invalid='ignore'):
            got = np.sum(wt * val) / np.sum(wt)
        assert np.isnan(got) == np.isnan(want)
        if not np.isnan(want):
            worst = max(worst, abs(got - want))
    print(f'levels seg_snr restated definition against the reference: worst |diff| = {worst:.3g} dB')
    assert worst < 1e-12


def test_reverb_bars_and_split_kinds():
    assert abs(rc.TOL_SRR - 3.5e-5) < 0.05e-5 and rc.TOL_DRR == 1e-10 and sg.TOL_SEG == 1e-9
    seen = set()
    for k, (Ld, Lh, n_sig, n_ch) in enumerate(rc.gen.REVERB_SHAPES):
        x, rir, rs, kinds, drr, srr = rc.golden_shape(k)
        for i in range(n_sig):
            for c in range(n_ch):
                sp = int(rc.split_def(rir[i, c], rc.n_direct(rs[i, c])))
                seen |= {'one'} if sp == 1 else set()
                seen |= {'inside_first'} if 1 < sp < 512 else set()
                seen |= {'at_512'} if sp == 512 else set()
                seen |= {'at_1024'} if sp == 1024 else set()
                seen |= {'inside_last'} if sp > ((Lh - 1) // 512) * 512 and sp < Lh - 1 else set()
                seen |= {'last_tap'} if sp == Lh - 1 else set()
    assert seen == set(rc.gen.SPLIT_KINDS), seen
    assert {rc.n_direct(v) for v in (0.0, 2.5, 20.0)} == {0, 40, 320}
    assert {(s[0], s[1]) for s in rc.gen.REVERB_SHAPES} == {(1500, 700), (1500, 1024), (1500, 1300), (512, 513), (1, 700), (600, 8192)}


def test_reverb_special_rows():
    rc.check_special_rows()


def test_reverb_definition_restated():
    """DRR and SRR of the fixture from float64 NumPy on the definition's split: the fixture is the definition the header documents."""
    worst = 0.0
    for k in (0, 3, 4):
        x, rir, rs, kinds, drr, srr = rc.golden_shape(k)
        for i in range(rir.shape[0]):
            for c in range(rir.shape[1]):
                sp = int(rc.split_def(rir[i, c], rc.n_direct(rs[i, c])))
                h, xd = rir[i, c].astype(np.float64), x[i].astype(np.float64)
                e = rc.tap_energies_def(rir[i, c], sp)
                d = 10 * np.log10(e[0] / e[1])
                s = 10 * np.log10(np.sum(np.convolve(xd, h[:sp]) ** 2) / np.sum(np.convolve(xd, h[sp:]) ** 2))
                worst = max(worst, abs(d - drr[i, c]), abs(s - srr[i, c]))
    print(f'levels reverb restated definition against the reference: worst |diff| = {worst:.3g} dB')
    assert worst < 1e-10


def test_ci_wp_and_bar_data_golden():
    sg.check_tables()


def test_names_of_the_reference_exist():
    from disco_amd import _lib, metrics, misc_utils
    from disco_amd.dataset_utils import rooms
    from disco_amd.speech_enhancement import results_io
    assert all(callable(getattr(metrics, nm)) for nm in ('seg_snr', 'reverb_ratios', 'ci_wp')) and callable(misc_utils.bar_data)
    assert callable(rooms.reverb_at_mics) and results_io.SEG_SNR_KEYS == ('seg_snr_in_cnv', 'seg_snr_out')
    assert {'disco_seg_snr', 'disco_rir_split', 'disco_reverb_energies'} <= set(_lib.PROTOTYPES)
