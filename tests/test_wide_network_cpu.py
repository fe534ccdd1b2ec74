"""The float64 oracle (oracle/tango_oracle.py) above 16 channels, against the REFERENCE'S OWN offline_tango on three wide networks
(tests/golden/tango_ref_wide.npz, make_golden_wide.py): P2 = 17, 32 and a ragged 19.  Inputs regenerated from the fixture's seeds
(tests/wide_checks.py:wide_scene), their checksum asserted first.  Scored per (node, bin) against the step-2 sensitivity
kappa = cond(Rnn) / (1 - d1/d0) stored with the fixture: the reference solves every pencil with complex64 LAPACK, so its own output
can only be trusted to ~eps32 x kappa.  With few frames per channel, wide networks have kappa ~ 1e4 .. 1e5 in most bins (the K - 1
compressed signals are nearly collinear in the noise statistics), so a fixed cut as in check_reference_scene_per_bin would keep
almost nothing: every bin is held to max(2e-4, 10 eps32 kappa) instead, and the bins with kappa <= KAPPA_SIGNAL together to 1e-3."""
import os

import numpy as np
import pytest

import parity_checks as pc
import wide_checks as wc
from oracle import tango_oracle as to

EPS32 = 5.96e-8
KAPPA_SIGNAL = 1e4


def wide_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'tango_ref_wide.npz'))


@pytest.mark.parametrize('scene', wc.WIDE_SCENES, ids=[s[0] for s in wc.WIDE_SCENES])
def test_oracle_matches_reference_wide(golden_dir, scene):
    name, K, mics, seed = scene
    g = wide_fixture(golden_dir)
    assert int(g[f'{name}_seed']) == seed
    y, s, n = wc.wide_scene(K, mics, seed)
    assert wc.checksum(y, s, n) == str(g[f'{name}_sha']), 'the regenerated inputs differ from the ones the reference was run on'
    o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    res = {}
    for key in g.files:
        for nm in ('yf', 'z_y'):
            if key.startswith(f'{name}_{nm}'):
                k = int(key[len(f'{name}_{nm}'):])
                kappa = g[f'{name}_kappa2'][k].astype(np.float64)
                got = np.asarray(o[nm][k])
                e = pc._per_bin_err(got, g[key])
                ratio = e / np.maximum(2e-4, 10 * EPS32 * kappa)
                well = kappa <= KAPPA_SIGNAL
                e_sig = pc.relerr(got[well], g[key][well]) if well.any() else 0.0
                res[key] = {'worst_ratio': float(ratio.max()), 'well_bins': int(well.sum()), 'well_signal': float(e_sig)}
                assert ratio.max() <= 1.0 and e_sig < 1e-3, (key, res[key])
    assert res, name
    print(res)
