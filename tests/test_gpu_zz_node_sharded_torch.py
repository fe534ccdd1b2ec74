"""Device-resident node-sharded driver on the MI355X (disco_amd/node_sharded.py:tango_enhance_node_sharded_torch): one-rank
RCCL group on the single GPU of the test box -- torch ROCm tensors as z / yf buffers, all_gather_into_tensor, the
iterated scheme with disco_filter_head -- against disco_tango_enhance_iterated.  The two-rank data flow is covered by
tests/test_sharding_gloo.py on CPU; 8-GPU runs are the driver's.  (File name sorts last: written when no GPU time was left
to try it, so it must not stand in front of the parity suite under `-x`.)"""
import pytest

import parity_checks as pc
from disco_amd import _lib
from disco_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_node_sharded_torch_one_rank_rccl():
    import torch
    lib = _lib.load()
    torch.cuda.set_device(0)
    errs = pc.check_node_sharded_torch_one_rank(lambda **cfg: Engine(lib=lib, **cfg), 'cuda:0', 'nccl', K=4, M=4, L=40000, iters=2)
    print(errs)


@pytest.mark.timeout(300)
def test_node_sharded_overlap_follows_parent():
    """overlap=True == overlap=False on a parent with mu != 1, another reference microphone, pinned tuning and another solver route."""
    import torch
    lib = _lib.load()
    torch.cuda.set_device(0)
    print(pc.check_node_sharded_overlap_follows_parent(lambda **cfg: Engine(lib=lib, **cfg), 'cuda:0', 'nccl', K=4, M=4, L=20000))


def _bench_process(args, timeout=600):
    """-> the finished `python bench.py args`, started plainly (no rank variables in its environment)."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    return subprocess.run([sys.executable, os.path.join(repo, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=timeout)


def _run_bench(args, timeout=600):
    """-> the FULL result (the side file `--detail` names) of `bench.py --full args`, after checking the ONE compact stdout line against it."""
    import json
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        detail = os.path.join(td, 'detail.json')
        p = _bench_process(args + ['--full', '--detail', detail], timeout=timeout)
        assert p.returncode == 0, p.stderr[-3000:]
        full = json.load(open(detail))
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and len(lines[0]) <= 6000, [len(l) for l in lines]
    line = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'scaling', 'dtype', 'config'):
        assert line[k] == full[k], k
    assert line['parity_sample']['ok'] == full['parity_sample']['ok'] and list(line)[-1] == 'summary'
    return full


@pytest.mark.timeout(900)
def test_bench_node_sharded_one_rank():
    """bench.py --shard nodes on ONE GPU: the node-sharded driver (staged kernels, all_gather_into_tensor over a 1-rank RCCL
    group) timed and parity-checked against the oracle like the default mode."""
    d = _run_bench(['--gpus', '1', '--shard', 'nodes', '--rooms', '6', '--length', '40000', '--steps', '2', '--warmup', '1',
                    '--no-cpu-baseline'])
    assert d['n_gpus'] == 1 and d['parity_sample']['ok'] and d['parity_sample']['worst_rel'] < 1e-4
    assert d['exchange']['gathers_per_step'] == 1 and d['exchange']['ms_per_gather'] is not None


@pytest.mark.timeout(600)
def test_bench_plain_times_the_headline_only(tmp_path):
    """`python bench.py` without --full: the headline is timed and its outputs are dumped, and nothing else runs -- no oracle check,
    no per-stage pass, no CPU baseline, no other configuration; the ONE line still carries the contract's keys."""
    import json
    import numpy as np
    p = _bench_process(['--gpus', '1', '--rooms', '6', '--length', '40000', '--steps', '2', '--warmup', '1',
                        '--dump-outputs', str(tmp_path / 'out'), '--detail', str(tmp_path / 'detail.json')])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['unit'] == 'node-frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f32' and line['n_gpus'] == 1
    c = line['config']
    assert abs(line['value'] * line['ms_per_step'] * 1e-3 / (c['rooms_per_gpu'] * c['nodes'] * c['frames']) - 1) < 1e-3
    assert line['roofline'] is None and line['cpu_baseline'] is None and 'parity_sample' not in line
    full = json.load(open(tmp_path / 'detail.json'))
    assert full['stages'] is None and full['parity_sample'] is None and 'configs' not in full
    enh = np.load(tmp_path / 'out' / 'enhanced.npy')
    assert enh.shape == (6, 4, 40000) and np.isfinite(enh).all()


@pytest.mark.timeout(900)
@pytest.mark.parametrize('shard', ['rooms', 'nodes'])
def test_bench_two_ranks_rccl(shard):
    """`python bench.py --gpus 2` started plainly: the script launches its own two ranks (one per GPU, RCCL).  --shard nodes
    splits the 4 nodes of every room 2 + 2 and exchanges z with a real two-rank all-gather over xGMI; rank 0's nodes are
    checked against the float64 oracle of the WHOLE room.  On a box with ONE GPU the job cannot run (two RCCL ranks cannot share a
    device): the launcher must refuse it before it starts a rank -- non-zero exit, the shortage named, no result line."""
    import torch
    args = ['--gpus', '2', '--shard', shard, '--rooms', '8', '--length', '40000', '--steps', '2', '--warmup', '1', '--no-cpu-baseline']
    have = torch.cuda.device_count()
    if have < 2:
        p = _bench_process(args, timeout=300)
        assert p.returncode != 0 and f'--gpus 2 but only {have} GPU(s) are visible' in p.stderr, (p.returncode, p.stderr[-2000:])
        assert not p.stdout.strip(), p.stdout[-500:]
        return
    d = _run_bench(args)
    assert d['n_gpus'] == 2 and d['parity_sample']['ok'] and d['parity_sample']['worst_rel'] < 1e-4
    if shard == 'nodes':
        assert d['exchange']['link_GBps'] is not None and d['scaling'] == 'strong'


@pytest.mark.timeout(1200)
def test_bench_two_ranks_bookkeeping_on_one_gpu():
    """The N > 1 bookkeeping of the plain bench line on a box with ONE GPU: two self-launched ranks, both computing on cuda:0, the
    control collectives over gloo (`--dist-backend gloo --single-device`; a functional test, not a measurement).  Every rank owns its
    own rooms and checks rooms of its own batch; the headline and every attached configuration carry both ranks' parity rows and the
    worst error over both; an attached configuration's value is the units of both ranks over the slower rank's time."""
    d = _run_bench(['--gpus', '2', '--dist-backend', 'gloo', '--single-device', '--rooms', '8', '--length', '40000', '--steps', '2',
                    '--warmup', '1', '--extras', 'C2,online1', '--no-cpu-baseline'], timeout=1100)
    assert d['n_gpus'] == 2 and d['config']['rooms_per_gpu'] == 8
    ps = d['parity_sample']
    assert ps['ok'] and ps['worst_rel_all_ranks'] < 1e-4 and len(ps['ranks']) == 2
    assert [r['first_room'] for r in ps['ranks']] == [0, 8] and [r['rank'] for r in ps['ranks']] == [0, 1]
    assert all(0 <= x < 8 for x in ps['ranks'][0]['rooms_checked']) and all(8 <= x < 16 for x in ps['ranks'][1]['rooms_checked'])
    assert set(d['configs']) == {'C2', 'online1'}
    for nm, v in d['configs'].items():
        assert 'error' not in v, (nm, v)
        assert len(v['seconds_per_rank']) == 2 and v['parity_sample']['ok'] and len(v['parity_sample']['ranks']) == 2, nm
        units = 2 * v['config']['rooms_per_gpu'] * v['config']['nodes'] * v['config']['frames'] * v['steps']
        assert abs(v['value'] - units / max(v['seconds_per_rank'])) < 1e-6 * v['value'], nm


@pytest.mark.timeout(1500)
@pytest.mark.parametrize('shard', ['rooms', 'nodes'])
def test_bench_four_ranks_bookkeeping_on_one_gpu(shard):
    """A many-rank job on a box with ONE GPU: four self-launched ranks, all computing on cuda:0, the collectives over gloo
    (`--dist-backend gloo --single-device`; functional, not a measurement -- RCCL with more than one rank has never run in this project,
    DESIGN section 6).  Four, not the eight of the driver's scaling run, so that at most five processes hold the one GPU at a time (this
    one and the ranks: under --single-device the launcher does not open the device); the eight-rank exchange bookkeeping runs on CPU
    (tests/test_sharding_gloo.py:test_bench_dry_collective_exchange_fields).
      rooms: every rank owns its own 2 rooms (first_room = 2 rank) and checks a room of its OWN batch; the line carries four parity rows.
      nodes: 4 nodes, ONE per rank (the exchange DISCO's algorithm performs): every step-2 pass all-gathers z over the four ranks and
             consumes it rank-major ([W][R][1][T][F], disco_set_z_blocks); every rank checks its node against the oracle of the WHOLE room."""
    W = 4
    common = ['--gpus', str(W), '--dist-backend', 'gloo', '--single-device', '--rooms', '2', '--length', '24000', '--steps', '1', '--warmup', '1',
              '--extras', 'none', '--no-cpu-baseline']
    if shard == 'rooms':
        d = _run_bench(common, timeout=1400)
        ps = d['parity_sample']
        assert d['n_gpus'] == W and d['scaling'] == 'weak' and len(ps['ranks']) == W
        assert [r['first_room'] for r in ps['ranks']] == [2 * r for r in range(W)]
        for r in ps['ranks']:
            assert all(2 * r['rank'] <= x < 2 * r['rank'] + 2 for x in r['rooms_checked']), r
    else:
        d = _run_bench(common + ['--shard', 'nodes', '--nodes', str(W), '--mics', '2'], timeout=1400)
        ps = d['parity_sample']
        assert d['n_gpus'] == W and d['scaling'] == 'strong' and len(ps['ranks']) == W
        assert d['exchange']['gathers_per_step'] == 1 and d['exchange']['bytes_per_peer_link_per_gather'] == 2 * 1 * d['config']['frames'] * 257 * 8
        assert '1 per rank' in d['config']['parallelism']
    assert ps['ok'] and ps['worst_rel_all_ranks'] < 1e-4, ps
