"""The bench line's contract, checked on CPU against the full result the final GPU pass committed (DETAIL below: what bench.py writes to
bench_detail.json): the ONE stdout line is bench.compact_line of it -- at most bench.LINE_LIMIT bytes (round 5's 20 kB line was not parsed
by the driver), the keys the driver reads first, the two objects the tier asks for (`roofline`, `cpu_baseline`) with their numbers, and
the compact `summary` -- the LAST key -- rebuilt here by bench.summary_rows from the full result's own fields."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LINE = os.path.join(REPO, 'profiles', 'r06_zz_bench_detail.json')       # the full result of round 6's final pass (what bench.py wrote beside its line)


def _line():
    """the full result (side file)"""
    return json.loads(open(LINE).read())


def test_stdout_line_is_small_and_carries_the_objects():
    import bench
    full = _line()
    line = bench.compact_line(full, 'bench_detail.json')
    text = json.dumps(line)
    assert len(text) <= bench.LINE_LIMIT <= 12_000, len(text)
    back = json.loads(text)
    assert list(back)[:12] == ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                               'dtype', 'data']
    assert list(back)[-1] == 'summary' and back['summary'] == full['summary'] and back['detail'] == 'bench_detail.json'
    assert back['roofline']['frac'] == full['roofline']['frac'] and back['roofline']['bound'] in ('hbm', 'mfma')
    assert back['roofline']['traffic'] == full['roofline']['traffic'] and back['roofline']['pipeline'] == full['roofline']['pipeline']
    assert back['cpu_baseline']['value'] > 0 and back['cpu_baseline']['kind'] in ('reference', 'port') and back['cpu_baseline']['cores'] >= 1
    assert back['cpu_baseline']['sample'] and back['cpu_baseline']['unit'] == 'node-frames/s'
    assert back['parity_sample']['ok'] is True and back['parity_sample']['worst_rel_all_ranks'] < 1e-4
    assert 'workload' in back['config'] and 'model' not in back['config']
    for k in ('configs', 'stages'):
        assert k not in back, k                             # they live in the side file
    # a line with every optional object at its largest still fits
    fat = dict(full, exchange={k: 1.23456789e9 for k in ('collective', 'gathers_per_step', 'bytes_received_per_rank_per_gather',
                                                         'bytes_per_peer_link_per_gather', 'ms_per_gather', 'link_GBps', 'timed')},
               graph={'ms_per_step': 1.0, 'pipeline_frac': 0.5})
    fat['roofline'] = dict(full['roofline'], kernel='k' * 400, sanity_errors=['x' * 500] * 4, traffic_note='y' * 900)
    fat['cpu_baseline'] = dict(full['cpu_baseline'], sample='s' * 3000)
    assert len(json.dumps(bench.compact_line(fat, 'bench_detail.json'))) <= bench.LINE_LIMIT


def test_contract_keys_and_objects():
    d = _line()
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data',
              'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['unit'] == 'node-frames/s' and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert 'workload' in d['config'] and 'model' not in d['config']
    rf, cb = d['roofline'], d['cpu_baseline']
    assert rf['bound'] in ('hbm', 'mfma') and rf['unit'] in ('GB/s', 'TFLOP/s') and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-3
    assert cb['kind'] in ('reference', 'port') and cb['cores'] >= 1 and cb['value'] > 0 and cb['sample']
    # value = the node-frames all ranks processed / the timed seconds
    c = d['config']
    units = c['rooms_per_gpu'] * d['n_gpus'] * c['nodes'] * c['frames']
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 / units - 1) < 1e-3


def test_summary_is_last_small_and_faithful():
    import bench
    d = _line()
    assert list(d)[-1] == 'summary'
    s = d['summary']
    assert len(json.dumps(s)) < 1500
    names = [k for k in s if k != '_cols']
    assert set(d['configs']) <= set(names) and len(names) == len(d['configs']) + 1
    head_name = [k for k in names if k not in d['configs']][0]
    rebuilt = bench.summary_rows(head_name, d, d.get('parity_sample'), d['configs'])
    assert rebuilt == s
    # the line the same run printed: the compact form of this very result
    printed = json.loads(open(os.path.join(REPO, 'profiles', 'r06_zz_bench_line.json')).read().strip().splitlines()[-1])
    assert printed['summary'] == s and printed['value'] == d['value'] and printed['roofline']['frac'] == d['roofline']['frac'] and len(json.dumps(printed)) <= bench.LINE_LIMIT
    # every workload row: ms, x real-time, pipeline fraction, kernel, its fraction, traffic ratio, parity
    for nm in names:
        row = s[nm]
        src = d if nm == head_name else d['configs'][nm]
        assert row[0] == round(src['ms_per_step'], 3) and row[1] == round(src['x_realtime'], 1)
        assert row[6] is not None and row[6] < 1e-4
    assert 'stream_x_realtime_by_hops' in s['online1'][7] and 'hipgraph' in s['C2'][7]


def test_flagged_bins_come_from_the_masks_alone():
    """bench.flagged_bins (the weight rule; bench.score_given_masks adds the bins whose float64 answer moves under a float32-class input
    perturbation): a bin is flagged when ANY (step, node) statistic of it has less than FLAG_WEIGHT frames of weight; flagged bins are scored
    against the distance the reference's own solve keeps from the oracle, the others at 1e-4 -- every sampled room, every bin is asserted (the
    scoring itself runs on the kernels in tests/test_kernels_emulated_wide.py::test_emu_saturating_masks and on the GPU)."""
    import numpy as np
    import bench
    rng = np.random.default_rng(0)
    good = [rng.uniform(0.05, 0.95, size=(5, 40)) for _ in range(2)]
    fb, w = bench.flagged_bins((good, good))
    assert fb.size == 0 and w > 1e-2
    bad = [m.copy() for m in good]
    bad[1][3, :] = 1.0 - 1e-6                                  # one bin saturated in every frame: sum_t (1 - m)^2 = 40e-12
    fb, w = bench.flagged_bins((good, bad))
    assert list(fb) == [3] and abs(w - 40e-12) < 1e-12 and w < bench.FLAG_WEIGHT
    worse = [m.copy() for m in good]
    worse[0][1, :] = 1e-7
    fb, _ = bench.flagged_bins((worse, bad))
    assert list(fb) == [1, 3]
    src = open(os.path.join(REPO, 'bench.py')).read()
    assert 'ILL_POSED' not in src and 'reported, not asserted' not in src


def test_dump_outputs_fixed_sample_within_budget(tmp_path):
    """--dump-outputs (bench.dump_outputs): float32 .npy files under the byte budget, the same rooms of every array, a seeded sample that
    is the same from run to run; all rooms when they fit, a seeded sample of elements when one room alone is over the budget."""
    import numpy as np
    import pytest
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = {'enhanced': torch.randn(50, 2, 1000, generator=g), 'mask': torch.rand(50, 2, 9, 17, generator=g, dtype=torch.float64)}
    per_room = 4 * (2 * 1000 + 2 * 9 * 17)

    def dump(d, budget):
        rooms = bench.dump_outputs(str(d), arrays, budget=budget)
        got = {nm: np.load(d / f'{nm}.npy') for nm in arrays}
        assert all(a.dtype == np.float32 for a in got.values()) and sum(a.nbytes for a in got.values()) <= budget
        return rooms, got

    rooms, got = dump(tmp_path / 'a', 10 * per_room + 5)
    assert len(rooms) == 10 and rooms == sorted(set(rooms)) and all(0 <= r < 50 for r in rooms)
    for nm, a in arrays.items():
        assert np.array_equal(got[nm], a[rooms].float().numpy())
    rooms2, got2 = dump(tmp_path / 'b', 10 * per_room + 5)
    assert rooms2 == rooms and all(np.array_equal(got[nm], got2[nm]) for nm in arrays)
    rooms, got = dump(tmp_path / 'c', 50 * per_room)
    assert rooms == list(range(50)) and np.array_equal(got['enhanced'], arrays['enhanced'].numpy())
    rooms, got = dump(tmp_path / 'd', per_room // 3)
    assert len(rooms) == 1 and got['enhanced'].ndim == 1 and got['enhanced'].size > 0
    assert np.isin(got['enhanced'], arrays['enhanced'][rooms[0]].numpy()).all()
    _, again = dump(tmp_path / 'e', per_room // 3)
    assert all(np.array_equal(got[nm], again[nm]) for nm in arrays)
    assert bench.parse_args(['--dump-outputs', str(tmp_path)]).dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])


def test_plain_run_times_the_headline_only():
    """Without --full the command times the headline and nothing else: no oracle check, no per-stage pass, no CPU baseline and no other
    configuration (an explicit --extras asks for --full), and its line is the compact line of that result.  --full runs all of it."""
    import pytest
    import bench
    for argv in ([], ['--config', 'C5'], ['--shard', 'nodes'], ['--extras', 'none']):
        a = bench.parse_args(argv)
        assert not a.full and a.extra_names == [] and a.no_parity and a.no_cpu_baseline and a.no_stage_timing, argv
    a = bench.parse_args(['--full'])
    assert a.extra_names == [n for n in bench.EXTRAS if n != 'C4_bf16'] and not (a.no_parity or a.no_cpu_baseline or a.no_stage_timing)
    assert bench.parse_args(['--full', '--config', 'C5']).extra_names == []
    assert bench.parse_args(['--full', '--extras', 'C2,C4_bf16', '--no-parity']).extra_names == ['C2', 'C4_bf16']
    with pytest.raises(SystemExit):
        bench.parse_args(['--extras', 'C2'])
    # what main() assembles from a plain run: the headline's own fields, nothing measured beside them
    d = _line()
    plain = {k: d[k] for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                               'vs_baseline', 'dtype', 'data', 'x_realtime', 'config')}
    plain.update(roofline=None, cpu_baseline=None, parity_sample=None, stages=None)
    plain['summary'] = bench.summary_rows('C3', plain, None, {})
    line = bench.compact_line(plain)
    assert list(line)[:12] == ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                               'dtype', 'data']
    assert all(line[k] == d[k] for k in ('metric', 'value', 'unit', 'ms_per_step', 'higher_is_better', 'dtype'))
    assert line['roofline'] is None and line['cpu_baseline'] is None and 'parity_sample' not in line and list(line)[-1] == 'summary'
    assert line['summary']['C3'][:2] == [round(d['ms_per_step'], 3), round(d['x_realtime'], 1)]
