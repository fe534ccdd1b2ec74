"""tango_ref_wide.npz: the reference's own `offline_tango` on three wide networks whose step-2 pencils exceed 16 channels
(P2 = max M_k + K - 1 = 17, 32 and 19; tests/wide_checks.py:WIDE_SCENES).  Same machinery as make_golden.py: the reference's function
bodies are taken from the reference tree at run time, nothing of it is copied.

The inputs are NOT stored (tens of MB at these channel counts): they are regenerated from the seeds by tests/wide_checks.py:wide_scene,
and the fixture keeps the seeds, a SHA-256 of the float32 inputs (the tests assert it first: a generator drift fails as such, not as a
parity error) and the reference's outputs for a subset of nodes (the file stays under 1 MiB).  Every scene has T >= 4 P2 frames.
Per (node, bin) the sensitivity of the step-2 pencil is stored too (condition of Rnn / relative gap of the top pair, from the float64
restatement), so that the tests can score per bin as check_reference_scene_per_bin does.
Run: python tests/golden/make_golden_wide.py"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# nodes whose outputs are kept, per scene: (yf nodes, z_y nodes)
KEEP = {'k16m2': ((0, 15), ()), 'k25m8': ((0,), ()), 'k12ragged': ((6,), (6,))}


def main():
    import make_golden as mg
    import make_golden_scenes as ms
    import wide_checks as wc
    from oracle import tango_oracle as to
    intern_filter, tf_mask, offline_tango, scratch = mg._load_reference()
    try:
        d = {'n_fft': np.array(wc.WIDE_N_FFT)}
        for name, K, mics, seed in wc.WIDE_SCENES:
            y, s, n = wc.wide_scene(K, mics, seed)
            # the reference reads its network size from module constants (tango.py:30-32, four nodes): set for this network
            offline_tango.__globals__.update(nb_ch=np.array(mics), nb_nodes=K, ref_mics=[0] * K)
            res = offline_tango(y, s, n, vads=['irm1', 'irm1'], mods=[None, None], mask_for_z='local')
            o = to.offline_tango_vec(y, s, n, vads=['irm1', 'irm1'], precision='f64', solver='eigh')
            c1, g1, c2, g2 = ms.sensitivity(o, K)
            d[f'{name}_seed'] = np.array(seed)
            d[f'{name}_sha'] = np.array(wc.checksum(y, s, n))
            d[f'{name}_kappa2'] = (c2 / np.maximum(1.0 - g2, 1e-300)).astype(np.float32)
            keep_yf, keep_z = KEEP[name]
            worst = 0.0
            for k in keep_yf:
                d[f'{name}_yf{k}'] = np.asarray(res[0][k]).astype(np.complex64)
                worst = max(worst, float(np.linalg.norm(res[0][k] - o['yf'][k]) / np.linalg.norm(o['yf'][k])))
            for k in keep_z:
                d[f'{name}_z_y{k}'] = np.asarray(res[3][k]).astype(np.complex64)
            print(f'{name}: K={K} P2={max(mics) + K - 1} T={o["yf"][0].shape[1]}; reference vs float64 restatement (kept yf, whole signal) '
                  f'{worst:.2e}; max kappa2 {float(d[f"{name}_kappa2"].max()):.3g}')
        np.savez_compressed(os.path.join(HERE, 'tango_ref_wide.npz'), **d)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


if __name__ == '__main__':
    main()
