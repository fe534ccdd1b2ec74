"""The helper kernels of mixed-length CRNN batches under the hipemu CPU emulator (no GPU), and offline_tango_rooms with CRNN masks through the
emulated library (tests/crnn_length_checks.py)."""
import numpy as np
import pytest

import crnn_length_checks as cl
import emu_build
from disco_amd import _engines, _lib


@pytest.fixture(scope='module')
def lib():
    return emu_build.load_emu()


@pytest.fixture()
def emulated_package(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', emu_build.load_emu())
    _engines._cache.clear()
    yield
    _engines._cache.clear()


@pytest.mark.parametrize('shape,frame_sets', [((3, 3, 2, 9, 17), ((9, 1, 4),)), ((2, 4, 4, 40, 257), ((40, 1), (20, 40)))])
def test_emu_crnn_features_rooms(lib, shape, frame_sets):
    print(cl.check_features_rooms(lib, 'cpu', *shape, frame_sets))


def test_emu_crnn_windows_rooms(lib):
    assert cl.check_windows_rooms(lib, 'cpu')


def test_emu_crnn_expand_rows(lib):
    assert cl.check_expand_rows(lib, 'cpu')


def test_emu_offline_tango_batched_takes_crnn_with_lengths(emulated_package):
    """The call that used to raise: 'crnn' at both steps with per-room lengths.  The masks of the frames a room does not have are zeros, and the
    step-1 masks of a room of the batch are those of the room run alone (float32 on the CPU both times)."""
    from disco_amd import synth
    from disco_amd.speech_enhancement.tango import offline_tango, offline_tango_rooms
    K, M, lengths = 2, 2, (6272, 5000)
    rooms = [synth.make_room_numpy(r, K=K, M=M, L=L)[:3] for r, L in enumerate(lengths)]
    mods = [cl.rand_model(1, 1, 'cpu'), cl.rand_model(K, 2, 'cpu')]
    res = offline_tango_rooms(rooms, vads=['crnn', 'crnn'], mods=mods)
    for r, L in enumerate(lengths):
        sep = offline_tango(*rooms[r], vads=['crnn', 'crnn'], mods=mods)
        for k in range(K):
            assert res[r][7][k].shape == (257, 1 + L // 256) and np.isfinite(res[r][0][k]).all()
            assert float(np.abs(res[r][7][k] - sep[7][k]).max()) < cl.ALONE_TOL, (r, k)
