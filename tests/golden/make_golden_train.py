#!/usr/bin/env python3
"""Golden fixture for the training path (disco_amd/dnn/data.py, losses.py, train.py, CRNN.get_loss_frames), produced by RUNNING THE
REFERENCE'S OWN CODE, exec'd from its source segments (the modules themselves cannot be imported: they pull in the whole training stack,
and dnn/engine/callbacks.py does not parse -- the '.' behind the docstring of early_stop_query is dropped from the text before it is
exec'd, nothing else).  Writes tests/golden/train_ref.npz: recorded data only (build container only).

  DiscoDataset.get_item_indices / get_subwindow / get_mask_frames   on an instance made with object.__new__ around a seeded bank
  reconstruction_loss                                               float64, with and without NaN entries
  get_loss_frames, get_x_for_loss, CRNN.get_loss_frames             'all' / 'mid' / 'last'
  SaveAndStop                                                       query sequences
"""
import ast
import os
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/disco_theque/dnn'


def segment(path, name, cls=None, patch=None):
    src = open(path).read()
    if patch:
        src = src.replace(*patch)
    body = ast.parse(src).body
    if cls:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name)
    return textwrap.dedent(ast.get_source_segment(src, node, padded=True))


def main():
    d = {}
    # ---- the data set -----------------------------------------------------------------------------------------------------------------
    ns = {'np': np, 'torch': torch, 'Dataset': object, 'os': os, 'FS': 16000, 'TRAIN_DUR': 11}
    exec(segment(f'{REF}/data/datasets.py', 'DiscoDataset'), ns)
    DiscoDataset = ns['DiscoDataset']
    K, S, N, F, T, W, hop = 4, 12, 3, 17, 40, 21, 8
    n_frames = np.array([40, 21, 33])
    rng = np.random.default_rng(2024)
    bank_u8 = rng.integers(0, 256, size=(S, N, F, T)).astype(np.uint8)       # magnitudes k / 16: exact in float32, small in the file
    data = bank_u8.astype(np.float32) / 16
    for k in range(N):
        data[:, k, :, n_frames[k]:] = 0
        bank_u8[:, k, :, n_frames[k]:] = 0

    def dataset(stack_axis, z_nodes):
        ds = object.__new__(DiscoDataset)
        ds.n_nodes, ds.win_len, ds.win_hop, ds.stack_axis, ds.z_nodes = K, W, hop, stack_axis, z_nodes
        ds.segs_to_load = [['-'] * N for _ in range(S)]
        ds.data, ds.n_frames = data, n_frames
        ds.win_per_seg = np.array([int((n - W) // hop + 1) for n in n_frames])
        ds.n_cum = np.cumsum([0] + list(ds.win_per_seg))
        return ds

    ds3, ds1 = dataset(2, 3), dataset(2, 1)
    d['bank_u8'], d['n_frames'], d['win_per_seg'], d['len'] = bank_u8, n_frames, ds3.win_per_seg, np.int64(len(ds3))
    items, jit, ks, ms = [], [], [], []
    for item in range(len(ds3)):
        for seed in range(100 * item, 100 * item + 3):
            np.random.seed(seed)
            k, m = ds3.get_item_indices(item)
            np.random.seed(seed)
            items.append(item), jit.append(np.random.randint(hop)), ks.append(k), ms.append(int(m))
    d['idx_item'], d['idx_jitter'], d['idx_k'], d['idx_m'] = map(np.array, (items, jit, ks, ms))

    def rows_of(mixt, k, m):                 # which bank rows the reference stacked, found by content
        out = []
        for ch in np.atleast_3d(mixt).reshape(-1, F, W):
            hit = [r for r in range(S) if np.array_equal(data[r, k, :, m:m + W], ch)]
            assert len(hit) == 1, hit
            out.append(hit[0])
        return out

    for tag, ds, cases in (('z3', ds3, [(i, i % K) for i in range(len(ds3))]), ('z1', ds1, [(i, (i + 2) % K) for i in range(4)])):
        tabs, wins, masks = [], [], []
        for item, local in cases:
            np.random.seed(7 + item)
            k, m = ds.get_item_indices(item)
            mixt, mask = ds.get_subwindow(local, k, int(m))
            assert np.array_equal(mask, ds.get_mask_frames(local, k, int(m)))
            tabs.append([k, int(m)] + rows_of(mixt, k, int(m)) + rows_of(mask, k, int(m)))
            wins.append((mixt * 16).astype(np.uint8)), masks.append((mask * 16).astype(np.uint8))
            assert np.array_equal(wins[-1].astype(np.float32) / 16, mixt)
        d[f'{tag}_tab'], d[f'{tag}_local'] = np.array(tabs, np.int32), np.array([c[1] for c in cases])
        d[f'{tag}_x_u8'], d[f'{tag}_y_u8'] = np.array(wins), np.array(masks)         # (B, C, F, T) / (B, F, T): the reference's orientation
    m_all = np.concatenate((d['z3_tab'][:, 1], d['z1_tab'][:, 1]))
    k_all = np.concatenate((d['z3_tab'][:, 0], d['z1_tab'][:, 0]))
    assert (m_all == 0).any() and (m_all == n_frames[k_all] - W).any() and (k_all == 1).any(), (k_all, m_all)
    assert set(d['z3_local']) == set(range(K)) == set(d['z1_local'])

    # ---- the loss ---------------------------------------------------------------------------------------------------------------------
    ns = {'torch': torch}
    exec(segment(f'{REF}/engine/losses.py', 'nanmean'), ns)
    exec(segment(f'{REF}/engine/losses.py', 'reconstruction_loss'), ns)
    for C in (1, 4):
        for Fq in (17,):
            est = rng.random((3, 15, Fq)).astype(np.float32)
            y = rng.random((3, 21, Fq)).astype(np.float32)
            x = (2 * rng.random((3, C, 21, Fq))).astype(np.float32)
            est_nan, x_nan = est.copy(), x.copy()
            est_nan[0, 3, 5], est_nan[2, 14, Fq - 1], x_nan[1, 0, 10, 2], x_nan[1, 0, 3, 0] = np.nan, np.nan, np.nan, np.nan
            t = f'loss_c{C}_f{Fq}'
            d[t + '_est'], d[t + '_y'], d[t + '_x'] = est.astype(np.float16), y.astype(np.float16), x.astype(np.float16)    # exact: see below
            est, y, x = (a.astype(np.float16).astype(np.float32) for a in (est, y, x))
            est_nan, x_nan = est_nan.astype(np.float16).astype(np.float32), x_nan.astype(np.float16).astype(np.float32)
            d[t + '_nan_est'] = np.argwhere(np.isnan(est_nan))
            d[t + '_nan_x'] = np.argwhere(np.isnan(x_nan))
            for part, (ff_in, ff_out, n_out) in {'all': (3, 0, 15), 'mid': (10, 7, 1), 'last': (17, 14, 1)}.items():
                for nan in (False, True):
                    e, xx = (est_nan, x_nan) if nan else (est, x)
                    val = ns['reconstruction_loss'](torch.from_numpy(y[:, ff_in:ff_in + n_out]).double(),
                                                    torch.from_numpy(e[:, ff_out:ff_out + n_out]).double(),
                                                    torch.from_numpy(xx[:, 0, ff_in:ff_in + n_out]).double())
                    d[f'{t}_{part}{"_nan" if nan else ""}'] = np.float64(val.item())

    # ---- frame selection ----------------------------------------------------------------------------------------------------------------
    ns = {'np': np, 'torch': torch}
    exec(segment(f'{REF}/utils.py', 'get_loss_frames'), ns)
    exec(segment(f'{REF}/utils.py', 'get_x_for_loss'), ns)
    exec('class M:\n    input_shape, x_out = (1, 21, 257), 15\n' + textwrap.indent(segment(f'{REF}/models/crnn.py', 'get_loss_frames', cls='CRNN'), '    '), ns)
    model = ns['M']()
    xs = {3: torch.from_numpy(rng.random((2, 21, 9)).astype(np.float32)), 4: torch.from_numpy(rng.random((2, 3, 21, 9)).astype(np.float32))}
    d['sel_x3'], d['sel_x4'] = xs[3].numpy(), xs[4].numpy()
    for part in ('all', 'mid', 'last'):
        d[f'frames_21_{part}'] = np.array(ns['get_loss_frames'](21, part))
        d[f'frames_15_{part}'] = np.array(ns['get_loss_frames'](15, part))
        d[f'crnn_frames_{part}'] = np.array(model.get_loss_frames(part))
        for dim, x in xs.items():
            d[f'sel{dim}_{part}_nomodel'] = ns['get_x_for_loss'](x, part, n_freq=7).numpy()
            d[f'sel{dim}_{part}_model0'] = ns['get_x_for_loss'](x, part, model=model, model_output=0, n_freq=7).numpy()
    d['frames_21_int5'] = np.array(ns['get_loss_frames'](21, 5))

    # ---- the callback -------------------------------------------------------------------------------------------------------------------
    ns = {'np': np}
    exec(segment(f'{REF}/engine/callbacks.py', 'SaveAndStop', patch=('for `self.patience` epochs""".', 'for `self.patience` epochs"""')), ns)
    values = np.array([0.9, 0.7, 0.8, 0.75, 0.71, 0.6, 0.6, 0.65, 0.66, 0.67])
    d['cb_values'] = values
    for tag, kw, vals in (('min', dict(patience=2, mode='min'), values), ('min_delta', dict(patience=1, mode='min', delta=0.05), values),
                          ('max', dict(patience=2, mode='max', delta=0.01), 1 - values)):
        cb = ns['SaveAndStop'](**kw)
        rec = []
        for v in vals:
            rec.append([int(cb.save_model_query(v)), cb.waited, int(cb.early_stop_query())])
        d[f'cb_{tag}'] = np.array(rec)

    out = os.path.join(HERE, 'train_ref.npz')
    np.savez_compressed(out, **d)
    print('wrote train_ref.npz', len(d), 'arrays,', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
