"""The marshalling helpers of disco_amd/engine.py against the recording stand-in of tools/engine_call_trace.py (no library, no emulator,
no GPU): a temporary buffer outlives the call that got its pointer, one object gives one pointer and one upload, None reaches C as NULL
where it should, device-resident arguments with caller-owned outputs cost no extra library call, a chunk walk steps every pointer by its
own stride -- and the source states each piece of marshalling once."""
import gc
import inspect
import re

import numpy as np

from disco_amd import _lib, engine
from disco_amd.engine import Engine
from tools.engine_call_trace import RecordingLib

R, K, M, LS = 2, 2, 2, 64


def _engine():
    lib = RecordingLib(_lib.PROTOTYPES)
    eng = Engine(rooms=R, nodes=K, mics=M, length=LS, n_fft=16, lib=lib)
    del lib.trace[:]
    return eng, lib


def _names(lib, frees=False):
    return [e[0] for e in lib.trace if frees or e[0] != 'disco_dev_free']


def _the(lib, name):
    found = [e for e in lib.trace if e[0] == name]
    assert len(found) == 1, (name, len(found))
    return found[0][1]


UPLOAD = ['disco_dev_alloc', 'disco_h2d', 'disco_sync']


def _inputs(eng):
    y = np.ones((R, K, M, LS), np.float32)
    return y, np.full((R, K, eng.T, eng.F), 0.5, np.float32), np.full((R, K, eng.T, eng.F), 0.5, np.float32)


def test_numpy_inputs_are_uploaded_once_and_outlive_the_call():
    eng, lib = _engine()
    y, mz, mz_equal = _inputs(eng)
    res = eng.tango_enhance(y, mz, mz)
    assert _names(lib) == UPLOAD * 2 + ['disco_dev_alloc'] * 3 + ['disco_tango_enhance']            # y, mask; out, z, yf
    a = _the(lib, 'disco_tango_enhance')
    assert a[2] == a[3] == ['dev', 1, 0] and a[1] == ['dev', 0, 0]                                   # one object, one pointer
    assert [a[4], a[5], a[6]] == [['dev', 2, 0], ['dev', 3, 0], ['dev', 4, 0]] and a[7:9] == [None, 0]
    call_at = lib.trace.index(['disco_tango_enhance', a])
    freed = {k: at for k, at, _ in lib.frees}
    assert sorted(freed) == [0, 1] and min(freed.values()) > call_at                                 # the uploads go after the call, the outputs stay
    assert [b.ptr for b in res] == [lib.starts[k] for k in (2, 3, 4)] and lib.live == {2, 3, 4}
    del res
    gc.collect()
    assert not lib.live and not lib.violations

    del lib.trace[:]
    eng.tango_enhance(y, mz, None, want_z=False, want_yf=False)                                      # None is the step-1 mask as well
    a = _the(lib, 'disco_tango_enhance')
    assert a[2] == a[3] and a[5] is None and a[6] is None and _names(lib).count('disco_h2d') == 2
    del lib.trace[:]
    eng.tango_enhance(y, mz, mz_equal, want_z=False, want_yf=False)                                  # equal values, another object: its own upload
    a = _the(lib, 'disco_tango_enhance')
    assert a[2] != a[3] and _names(lib).count('disco_h2d') == 3 and not lib.violations


def test_device_inputs_and_a_caller_owned_output_cost_one_library_call():
    eng, lib = _engine()
    y, mz = (eng.to_device(a, np.float32)[1] for a in _inputs(eng)[:2])
    out = eng.empty((R, K, LS), np.float32)
    del lib.trace[:]
    got, z, yf = eng.tango_enhance(y, mz, out=out, want_z=False, want_yf=False)
    assert got is out and z is None and yf is None
    assert _names(lib, frees=True) == ['disco_tango_enhance']
    assert _the(lib, 'disco_tango_enhance')[1:5] == [['dev', 0, 0], ['dev', 1, 0], ['dev', 1, 0], ['dev', 2, 0]]
    del lib.trace[:]
    got, z, yf = eng.tango_enhance(y, mz, out=out)
    assert got is out and _names(lib, frees=True) == ['disco_dev_alloc', 'disco_dev_alloc', 'disco_tango_enhance']
    import torch
    ty, tm, to = (lib.note_tensor(torch.zeros(s)) for s in ((R, K, M, LS), (R, K, eng.T, eng.F), (R, K, LS)))
    del lib.trace[:]
    assert eng.tango_enhance(ty, tm, out=to, want_z=False, want_yf=False)[0] is to
    assert _names(lib, frees=True) == ['disco_tango_enhance']
    assert _the(lib, 'disco_tango_enhance')[1:5] == [['tensor', 0, 0], ['tensor', 1, 0], ['tensor', 1, 0], ['tensor', 2, 0]]
    assert not lib.violations


def test_tango_reference_passes_none_as_null():
    eng, lib = _engine()
    y, mz, mw = _inputs(eng)
    eng.tango_reference(y, y, y, mask_z=mz, mask_w=None, steps=1)
    a = _the(lib, 'disco_tango_reference')
    assert a[1] is not None and a[4] is not None and a[5] is None                                   # the oracle mask, not mask_z
    del lib.trace[:]
    eng.tango_reference(y, y, y, mask_z=mz, mask_w=mz, steps=1)
    a = _the(lib, 'disco_tango_reference')
    assert a[4] == a[5] and a[4] is not None and _names(lib).count('disco_h2d') == 4
    del lib.trace[:]
    eng.tango_reference(y, y, y, mask_z=None, mask_w=mw, steps=1)
    a = _the(lib, 'disco_tango_reference')
    assert a[4] is None and a[5] is not None
    del lib.trace[:]
    eng.tango_reference(y, y, y, steps=1)
    a = _the(lib, 'disco_tango_reference')
    assert a[4] is None and a[5] is None and not lib.violations


def test_pair_stats_of_one_object_uploads_it_once():
    eng, lib = _engine()
    a = np.ones((3, LS), np.float32)
    eng.pair_stats(a, a)
    args = _the(lib, 'disco_pair_stats')
    assert args[1] == args[2] and _names(lib) == UPLOAD + ['disco_dev_alloc', 'disco_pair_stats']
    del lib.trace[:]
    eng.pair_stats(a, a.copy(), stop=np.array([10, 20, 30]))
    args = _the(lib, 'disco_pair_stats_spans')
    assert args[1] != args[2] and _names(lib) == UPLOAD * 3 + ['disco_dev_alloc', 'disco_pair_stats_spans'] and not lib.violations


def test_bss_eval_walks_five_sets_in_chunks_of_two():
    eng, lib = _engine()
    n, nsrc, n_est, L = 5, 2, 3, LS
    refs = np.arange(n * nsrc * L, dtype=np.float32).reshape(n, nsrc, L)                             # host: sliced and uploaded per chunk
    ests = eng.empty((n, n_est, nsrc, L), np.float32)                                                # device: read in place
    del lib.trace[:]
    energies, status = eng.bss_eval(refs, ests, stop=np.array([10, 20, 30, 40, 64]), flen=8, budget_bytes=2 * lib.per_item + 999)
    assert energies.shape == (n, n_est, nsrc, 4) and status.shape == (n,)
    assert [e[1][1] for e in lib.trace if e[0] == 'disco_bss_workspace_bytes'] == [1, 2]             # the size of one set, then of a chunk
    stop_alloc, ws_alloc = 1, 2                                                                      # allocation 0 is `ests`
    assert lib.sizes[stop_alloc] == 4 * n and lib.sizes[ws_alloc] == 8 * (2 * lib.per_item // 8 + 1)
    calls = [e[1] for e in lib.trace if e[0] == 'disco_bss_eval_spans']
    assert [c[3] for c in calls] == [2, 2, 1]
    for c, i0 in zip(calls, (0, 2, 4)):
        assert c[1][0] == 'dev' and c[1][1] > ws_alloc and c[1][2] == 0                              # this chunk's upload of refs
        assert lib.sizes[c[1][1]] == 4 * c[3] * nsrc * L
        assert c[2] == ['dev', 0, 4 * i0 * n_est * nsrc * L] and c[8] == ['dev', stop_alloc, 4 * i0]
        assert c[13] == ['dev', ws_alloc, 0] and c[14] == lib.sizes[ws_alloc]
    h2d = [e for e in lib.trace if e[0] == 'disco_h2d']
    assert [e[1][3] for e in h2d] == [4 * n] + [4 * m * nsrc * L for m in (2, 2, 1)]
    assert not lib.violations
    gc.collect()
    assert lib.live == {0}                                                                           # every temporary is gone, `ests` is the caller's

    del lib.trace[:]
    eng.bss_eval(eng.empty((n, nsrc, L), np.float32), np.zeros((n, n_est, nsrc, L), np.float32), flen=8, budget_bytes=2 * lib.per_item)   # the other way round
    calls = [e[1] for e in lib.trace if e[0] == 'disco_bss_eval']
    assert [c[3] for c in calls] == [2, 2, 1] and [c[1][2] for c in calls] == [4 * i0 * nsrc * L for i0 in (0, 2, 4)]
    assert len({c[1][1] for c in calls}) == 1 and all(c[2][2] == 0 for c in calls) and not lib.violations


def test_engine_states_each_piece_of_marshalling_once():
    src = inspect.getsource(engine)
    assert src.count('mask_w is None or mask_w is mask_z') <= 1
    assert len(re.findall(r'\bif out is None\b', src)) <= 1
    assert len(re.findall(r'(?<!not )isinstance\(\w+, np\.ndarray\)', inspect.getsource(Engine))) <= 1      # host or device, in the chunk walk
    assert '.ptr if ' not in src.replace(inspect.getsource(engine._ptr), '')
