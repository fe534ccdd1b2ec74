#!/usr/bin/env python3
"""Golden fixture for the acceptance rule of the meeting-room generator (tests/meeting_checks.py), produced by RUNNING THE REFERENCE'S OWN
CODE out of dataset_generation/gen_meetit/convolve_signals.py:
    get_value_range (43-56), check_sir_validity (94-111), and the three assignments of simulate_room that build the SIR classes (150-152).
The module imports soundfile, pyroomacoustics, mir_eval and ipdb (all absent), so the two function sources and the three statements are
taken with `ast` and executed at run time; nothing of them is written here.  check_sir_validity counts with plt.hist: matplotlib runs on
its non-interactive 'Agg' backend.  The loop around it is the one at :271-289 -- an accepted room's SIRs are appended to the history of
every source before the next room is judged.
Sequences (S sources, n_rirs_per_proc, delta_sir): SIRs drawn at random; a run that fills one class until it refuses; rooms that fail each
rule alone (a difference above delta_sir in either order and under every roll, the first SIR below the lowest and above the highest
class), and rooms on which only the first source decides.  No SIR equals a class edge: the reference indexes an empty array when the
first SIR is exactly the lowest edge.
The fixture holds arrays only.  Runs only in the build container.      python -B tests/golden/make_golden_meeting.py
"""
import ast
import os
import sys

import matplotlib
matplotlib.use('Agg')
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = os.environ.get('DISCO_REFERENCE', '/root/reference')
PATH = os.path.join(REF, 'dataset_generation/gen_meetit/convolve_signals.py')


def reference_pieces():
    src = open(PATH).read()
    body = ast.parse(src).body
    ns = {'np': np, 'plt': plt}
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in ('get_value_range', 'check_sir_validity'):
            exec(ast.get_source_segment(src, node), ns)
    sim = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == 'simulate_room')
    wanted = ('n_classes', 'bin_level', 'sir_classes')
    stmts = [ast.get_source_segment(src, n) for n in sim.body
             if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in wanted]
    assert len(stmts) == 3, stmts

    def classes(n_rirs_per_proc):
        loc = dict(ns, n_rirs_per_proc=n_rirs_per_proc)
        exec('\n'.join(stmts), loc)
        return loc['sir_classes']
    return ns['get_value_range'], ns['check_sir_validity'], classes


def run_loop(check, classes, sirs, n_rirs, delta):
    """The loop at :271-289 on given SIRs instead of drawn rooms."""
    S = sirs.shape[1]
    past = [[] for _ in range(S)]
    verdicts = []
    for cur in sirs:
        ok = check(cur, past, classes(n_rirs), delta_sir=delta)
        plt.close('all')
        verdicts.append(bool(ok))
        if ok:
            for k in range(S):
                past[k].append(cur[k])
    return np.array(verdicts), past


def sequences():
    rng = np.random.default_rng(77)
    off = lambda a: np.where(np.abs(a - np.round(a)) < 1e-3, a + 0.01, a)    # keep clear of the integer class edges
    seq = {}
    for S, n_rirs, delta in ((2, 8, 2), (3, 8, 2), (4, 16, 2), (2, 4, 1), (3, 5, 3)):
        first = rng.uniform(0.5, 15.5, 60)
        rest = first[:, None] + rng.uniform(-1.6 * delta, 1.6 * delta, (60, S - 1))
        seq[f'draw_S{S}_n{n_rirs}_d{delta}'] = (off(np.concatenate([first[:, None], rest], axis=1)), n_rirs, delta)
    # one class filled: level ceil(4 / 4) = 1 and ceil(9 / 4) = 3; the strict comparison admits level + 1 rooms
    for n_rirs in (4, 9):
        a = np.stack([rng.uniform(5.2, 7.8, 9), rng.uniform(5.2, 7.0, 9)], axis=1)
        a[:, 1] = a[:, 0] + rng.uniform(-1.5, 1.5, 9)
        b = np.array([[9.1, 9.5], [6.3, 6.1], [3.3, 3.0], [6.6, 7.0]])
        seq[f'fill_n{n_rirs}'] = (off(np.concatenate([a, b])), n_rirs, 2)
    # each rule alone (S = 2 and 3): the difference in either order, under the second roll only, a negative difference of any size; the range of
    # the first source alone (the others may leave it)
    seq['rules_S2'] = (np.array([[6.0, 3.9], [3.9, 6.1], [6.0, 4.1], [4.1, 6.0], [1.9, 2.5], [14.1, 13.5], [2.1, 1.0], [13.9, 15.2], [13.9, 16.1],
                                 [2.05, 4.04], [2.05, 4.06]]), 40, 2)
    seq['rules_S3'] = (np.array([[6.0, 5.0, 3.9], [3.9, 5.0, 6.0], [5.0, 3.9, 6.0], [5.0, 6.0, 3.9], [6.0, 5.0, 4.1], [1.5, 2.5, 3.0], [14.5, 13.5, 13.0],
                                 [7.0, 8.9, 7.5], [7.0, 9.1, 7.5], [10.5, 8.6, 12.4], [10.5, 8.4, 12.4]]), 40, 2)
    # the history of the first source alone is counted: second-source SIRs crowd a class the first source never enters
    seq['first_only'] = (off(np.stack([np.tile([3.5, 9.5], 6)[:11], np.tile([4.9, 8.2], 6)[:11]], axis=1)), 4, 2)
    return seq


def main():
    get_value_range, check, classes = reference_pieces()
    out = {}
    for name, (sirs, n_rirs, delta) in sequences().items():
        sirs = np.asarray(sirs, np.float64)
        assert np.all(np.abs(sirs[:, 0] - 2.0) > 1e-6)
        verdicts, past = run_loop(check, classes, sirs, n_rirs, delta)
        out[f'sirs_{name}'], out[f'valid_{name}'] = sirs, verdicts
        out[f'args_{name}'] = np.array([n_rirs, delta])
        out[f'past0_{name}'] = np.array(past[0], np.float64)
        print(name, 'accepted', int(verdicts.sum()), 'of', len(verdicts))
    cls = classes(10)
    out['class_edges'] = np.array([[int(v) for v in k.split('-')] for k in cls])
    out['class_level_n10'] = np.array(list(cls.values()), np.float64)
    args = [(i, n, 0, 20, 5) for n in (1, 5, 7, 100) for i in range(0, n + 1)] + \
           [(i, 12, -3.5, 9.0, nb) for nb in (1, 3, 4, 7) for i in (0, 1, 3, 5, 11, 12)] + [(3, 10, 2, 14, 4), (9, 10, 2, 14, 4)]
    out['gvr_args'] = np.array(args, np.float64)
    out['gvr_out'] = np.stack([get_value_range(int(i), int(n), vmin, vmax, int(nb)) for i, n, vmin, vmax, nb in args])
    path = os.path.join(HERE, 'meeting_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote meeting_ref.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
