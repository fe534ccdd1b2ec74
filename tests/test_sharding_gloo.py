"""The N>1 path of bench.py on CPU: two gloo ranks shard rooms with no data-path collective; the only
communication is the barrier / max-time / unit-sum of the timing contract (disco_amd/dist.py)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from disco_amd import dist as dd


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dd.init('gloo', rank, world)
    lo, hi = dd.room_range(rank, world, 5)
    # stand-in workload: each rank "processes" its rooms; rank 1 is slower
    units = (hi - lo) * 4 * 626
    seconds = 0.010 * (1 + rank)
    dist.barrier()
    value, tmax = dd.whole_job_throughput(units, seconds, world)
    # room ids must tile [0, world*5) without overlap
    ids = torch.zeros(world * 5, dtype=torch.int64)
    ids[lo:hi] = 1
    dist.all_reduce(ids)
    q.put((rank, lo, hi, value, tmax, ids.tolist()))
    dist.destroy_process_group()


def test_two_rank_room_sharding_and_timing_contract():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world, 120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [(r[1], r[2]) for r in res] == [(0, 5), (5, 10)]
    for r in res:
        assert r[5] == [1] * 10                                 # disjoint cover
        assert r[4] == pytest.approx(0.020)                     # max over ranks
        assert r[3] == pytest.approx(2 * 5 * 4 * 626 / 0.020)   # whole-job units / max time
    assert res[0][3] == res[1][3]


def test_split_rooms_balanced():
    for total, world in [(1000, 8), (1001, 8), (7, 8), (256, 3)]:
        parts = dd.split_rooms(total, world)
        assert parts[0][0] == 0 and parts[-1][1] == total
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1


def _collect(procs, q, world, timeout=600):
    """Results of all ranks; fails at once (instead of waiting out the timeout) when a rank dies."""
    import queue
    import time
    res, t0 = [], time.time()
    while len(res) < world:
        try:
            res.append(q.get(timeout=1.0))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() - t0 > timeout:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                raise AssertionError(f'rank(s) failed (exit codes {dead}) or timed out')
    return sorted(res)


def _prebuild_emu():
    """Build the emulated test library once in the parent, so the two ranks never compile it concurrently."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import emu_build
    emu_build.build_emu()


# ---- node-sharded mode: the z all-gather between the two steps (tango.py:378-386) over a real process group ------------
def _node_worker(rank, world, port, q):
    import numpy as np
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dd.init('gloo', rank, world)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import emu_build                                        # kernel sources under the hipemu CPU emulator (test tooling)
    from disco_amd import synth
    from disco_amd.engine import Engine
    from disco_amd.node_sharded import node_range, tango_enhance_node_sharded, torch_all_gather
    from oracle import tango_oracle as to
    R, K, M, L = 1, 2, 2, 4096
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    o = to.offline_tango_vec(y[0], s[0], n[0], vads=['irm1', 'irm1'], precision='f64', solver='eigh')
    k0, kl = node_range(rank, world, K)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=emu_build.load_emu())
    eng.set_node_shard(k0, kl)
    mask = np.stack([o['masks_z'][k].T for k in range(k0, k0 + kl)])[None].astype(np.float32)       # (1, kl, T, F)
    out, yf, z_all = tango_enhance_node_sharded(eng, y[:, k0:k0 + kl], mask, mask, torch_all_gather(world))
    err_z = max(float(np.linalg.norm(z_all[0, k].T - o['z_y'][k]) / np.linalg.norm(o['z_y'][k])) for k in range(K))
    err_yf = max(float(np.linalg.norm(yf.numpy()[0, i].T - o['yf'][k0 + i]) / np.linalg.norm(o['yf'][k0 + i])) for i in range(kl))
    q.put((rank, err_z, err_yf))
    dist.destroy_process_group()


def test_node_sharded_all_gather_two_ranks():
    """Two gloo ranks, one node each: step 1 local, all-gather of z, step 2 local -- both ranks match the float64 oracle
    (every rank sees ALL z after the gather; its own filtered output covers its own node)."""
    _prebuild_emu()
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_node_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, err_z, err_yf in res:
        assert err_z < 1e-5 and err_yf < 1e-5, (rank, err_z, err_yf)


def _node_worker_torch(rank, world, port, q):
    """The device-resident driver (torch tensors in, torch.distributed all_gather_into_tensor for z), 2 iterations: on the
    emulated build 'device' memory is host memory, so CPU tensors + gloo exercise the same code RCCL runs on the GPUs."""
    import numpy as np
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dd.init('gloo', rank, world)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import emu_build
    from disco_amd import synth
    from disco_amd.engine import Engine
    from disco_amd.node_sharded import node_range, tango_enhance_node_sharded_torch
    from oracle import tango_oracle as to
    R, K, M, L = 2, 2, 2, 1280
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    k0, kl = node_range(rank, world, K)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=emu_build.load_emu())
    eng.set_node_shard(k0, kl)
    res = {}
    for iters in (1, 2):
        os_ = [to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], precision='f64', solver='eigh', extra_iters=iters - 1)
               for r in range(R)]
        mask = np.stack([np.stack([o['masks_z'][k].T for k in range(k0, k0 + kl)]) for o in os_]).astype(np.float32)
        yt = torch.from_numpy(np.ascontiguousarray(y[:, k0:k0 + kl]))
        mt = torch.from_numpy(mask)
        out, yf, z_all = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters)
        assert isinstance(yf, torch.Tensor) and isinstance(z_all, torch.Tensor) and z_all.shape == (R, K, eng.T, eng.F)
        yf = yf.numpy()
        err = max(float(np.linalg.norm(yf[r, i].T - os_[r]['yf'][k0 + i]) / np.linalg.norm(os_[r]['yf'][k0 + i]))
                  for r in range(R) for i in range(kl))
        # every rank must hold the same gathered z, in global node order
        chk = torch.view_as_real(z_all).double().sum(dim=(0, 2, 3)).contiguous()
        ref = chk.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(chk, ref)
        res[iters] = err
    q.put((rank, res[1], res[2]))
    dist.destroy_process_group()


def test_node_sharded_device_resident_iterated_two_ranks():
    """tango_enhance_node_sharded_torch with 1 and 2 step-2 iterations (one all-gather each) on two gloo ranks against the
    float64 oracle of the same definition (offline_tango_vec(extra_iters=...))."""
    _prebuild_emu()
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_node_worker_torch, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, e1, e2 in res:
        assert e1 < 1e-5 and e2 < 1e-4, (rank, e1, e2)


def _node_worker_one_pass(rank, world, port, q):
    """A shape whose final filter + iSTFT run as ONE pass on the gathered z (disco_apply_istft_fused: 4 nodes x 4 mics, two nodes per rank):
    the kernel reads the z of all nodes in the rank-major blocks the all-gather delivers; two half-batches with asynchronous gathers
    (overlap=True), caller-owned filter arrays; with and without the filtered spectra."""
    import numpy as np
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dd.init('gloo', rank, world)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import emu_build
    from disco_amd import synth
    from disco_amd.engine import Engine
    from disco_amd.node_sharded import node_range, tango_enhance_node_sharded_torch
    from oracle import stft_oracle as so
    from oracle import tango_oracle as to
    R, K, M, L = 3, 4, 4, 2560
    y, s, n = synth.make_rooms_numpy(R, K=K, M=M, L=L)
    k0, kl = node_range(rank, world, K)
    eng = Engine(rooms=R, nodes=K, mics=M, length=L, lib=emu_build.load_emu())
    eng.set_node_shard(k0, kl)
    res = {}
    for iters in (1, 2):
        os_ = [to.offline_tango_vec(y[r], s[r], n[r], vads=['irm1', 'irm1'], precision='f64', solver='eigh', extra_iters=iters - 1)
               for r in range(R)]
        mask = np.stack([np.stack([o['masks_z'][k].T for k in range(k0, k0 + kl)]) for o in os_]).astype(np.float32)
        yt = torch.from_numpy(np.ascontiguousarray(y[:, k0:k0 + kl]))
        mt = torch.from_numpy(mask)
        out, yf, z_all = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters, overlap=True)
        eng.stage_timing(True)                              # (the overlapped form runs on child engines: the stages are read off the plain form)
        out_p, _, _ = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters, overlap=False)
        rep = eng.stage_report()
        eng.stage_timing(False)
        assert 'apply2_istft' in rep and 'istft' not in rep, sorted(rep)
        assert float((torch.as_tensor(out_p) - torch.as_tensor(out)).abs().max()) < 1e-5
        out_b, yf_b, _ = tango_enhance_node_sharded_torch(eng, yt, mt, mt, iters=iters, want_yf=False, overlap=True)
        assert yf is not None and yf_b is None and torch.equal(torch.as_tensor(out), torch.as_tensor(out_b))
        outn = out.numpy() if hasattr(out, 'numpy') else np.asarray(out)
        err = 0.0
        for r in range(R):
            for i in range(kl):
                ref = so.istft(os_[r]['yf'][k0 + i], L, work_dtype=np.float64)
                err = max(err, float(np.linalg.norm(outn[r, i] - ref) / np.linalg.norm(ref)))
                e_yf = float(np.linalg.norm(yf.numpy()[r, i].T - os_[r]['yf'][k0 + i]) / np.linalg.norm(os_[r]['yf'][k0 + i]))
                err = max(err, e_yf)
        res[iters] = err
    q.put((rank, res[1], res[2]))
    dist.destroy_process_group()


def test_node_sharded_one_pass_final_two_ranks():
    """Two gloo ranks with two of a room's four 4-mic nodes each: step 2 ends in the one-pass filter + iSTFT on the gathered z; samples and
    filtered spectra against the float64 oracle, 1 and 2 step-2 iterations."""
    _prebuild_emu()
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_node_worker_one_pass, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(procs, q, world)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for rank, e1, e2 in res:
        assert e1 < 2e-5 and e2 < 1e-4, (rank, e1, e2)


def test_bench_self_launches_ranks():
    """`python bench.py --gpus 2` started plainly (no torchrun, no WORLD_SIZE) must become TWO ranks: the launcher of
    disco_amd/dist.py:launch_ranks, exercised on CPU with gloo (`--selftest-launch` skips the GPU work, nothing else)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '2', '--selftest-launch'], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    # stdout carries the ONE JSON line and nothing else (descriptor 1 is handed to stderr for libraries: RCCL prints a version block from C stdio)
    assert len(p.stdout.strip().splitlines()) == 1, p.stdout[-500:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and lines[0]['n_gpus'] == 2                      # one line, from rank 0, of a 2-rank job
    assert lines[0]['value'] == pytest.approx((1000.0 + 2000.0) / 0.6)     # sum of units / max of times over the ranks
    # EVERY rank checks rooms of its own batch; the line carries each rank's rooms / device and the worst error over all ranks
    ps = lines[0]['parity_sample']
    assert ps['worst_rel_all_ranks'] == pytest.approx(2e-6) and ps['worst_rel'] == pytest.approx(1e-6) and ps['ok']
    assert [r['rank'] for r in ps['ranks']] == [0, 1] and [r['device'] for r in ps['ranks']] == [0, 1]
    assert ps['ranks'][0]['rooms_checked'] == [0, 4, 9] and ps['ranks'][1]['first_room'] == 10
    assert len(ps['ranks'][1]['rooms_checked']) == 1 and 10 <= ps['ranks'][1]['rooms_checked'][0] < 20
    # a world size that contradicts --gpus is an error, not a silent single-rank run
    p = subprocess.run([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '1', '--selftest-launch'],
                       env=dict(env, RANK='0', WORLD_SIZE='2', LOCAL_RANK='0'), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and 'WORLD_SIZE' in (p.stderr + p.stdout)


@pytest.mark.parametrize('world,nodes,iters', [(2, 4, 2), (4, 8, 1), (8, 8, 1)])
def test_bench_dry_collective_exchange_fields(world, nodes, iters):
    """`python bench.py --gpus W --shard nodes --dry-collective` (round-5 VERDICT item 9): W self-launched gloo ranks run the z exchange of the
    node-sharded step on CPU tensors of the real per-rank size -- `iters` all-gathers per step into the rank-major buffer, every block
    checked on every rank -- and rank 0 prints the `exchange` object of the line: bytes per rank and per peer link, ms per gather.
    Bookkeeping only: no RCCL communicator with more than one rank has run in this project."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    R, L = 3, 8000
    p = subprocess.run([sys.executable, os.path.join(repo, 'bench.py'), '--gpus', str(world), '--shard', 'nodes', '--dry-collective', '--rooms', str(R),
                        '--nodes', str(nodes), '--length', str(L), '--steps', '2', '--warmup', '1', '--iters', str(iters)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    d = lines[0]
    T, F, Kl = 1 + L // 256, 257, nodes // world
    ex = d['exchange']
    assert d['n_gpus'] == world and d['scaling'] == 'strong' and d['blocks_wrong'] == 0 and d['gathers_timed'] == 2 * iters
    assert d['config'] == {'rooms': R, 'nodes': nodes, 'nodes_per_rank': Kl, 'frames': T, 'bins': F, 'iters': iters}
    assert ex['gathers_per_step'] == iters and ex['overlap'] is False and 'DRY RUN' in ex['timed']
    assert ex['bytes_per_peer_link_per_gather'] == R * Kl * T * F * 8
    assert ex['bytes_received_per_rank_per_gather'] == (world - 1) * ex['bytes_per_peer_link_per_gather'] == R * (nodes - Kl) * T * F * 8
    assert ex['ms_per_gather'] > 0 and ex['link_GBps'] == pytest.approx(ex['bytes_per_peer_link_per_gather'] / (ex['ms_per_gather'] * 1e-3) / 1e9)
    # the compact line keeps exactly these fields of the object
    import bench
    keep = ('collective', 'gathers_per_step', 'bytes_received_per_rank_per_gather', 'bytes_per_peer_link_per_gather', 'ms_per_gather', 'link_GBps', 'timed')
    assert all(k in ex for k in keep) and 'exchange' in open(bench.__file__).read()


def test_launch_ranks_propagates_failure(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text('import os, sys, time\nr = int(os.environ["RANK"])\nif r == 1:\n    sys.exit(7)\ntime.sleep(30)\n')
    import time
    t0 = time.time()
    rc = dd.launch_ranks(str(script), [], 2, timeout=60)
    assert rc == 7 and time.time() - t0 < 20          # rank 0 was terminated instead of waiting out its sleep
