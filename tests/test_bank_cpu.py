"""The training bank from rooms, what needs neither the library nor a GPU (tests/bank_checks.py): from_rooms refuses bad inputs with
ValueError before anything is launched, write_post_dataset's folders and file names against the reference's literal layout, get_input_lists
and get_dset."""
import bank_checks as bc


def test_from_rooms_refuses_bad_inputs_before_any_launch():
    assert bc.check_bad_inputs()


def test_post_dataset_file_names(tmp_path):
    assert bc.check_file_names(tmp_path)


def test_input_lists():
    assert bc.check_input_lists()


def test_dset_and_directory_names():
    assert bc.check_dset_names()


def test_restatement_of_the_fill():
    """The NumPy restatement the kernel is held to, on a case worked by hand: K = 1, two rooms into segments 1 and 2 of 4."""
    import numpy as np
    c = bc.make_case(R=2, K=1, T=3, F=2, M=1, mic=0, z=(True, False), frames=(3, 2), skip=1, N=4, Tb=3, seg0=1, specials=False)
    want, is_mag = bc.restate(c)
    assert want.shape == (3, 4, 3, 2) and list(is_mag) == [True, True, False]
    assert (want[:, [0, 3]] == bc.SENTINEL).all()
    assert np.array_equal(want[0, 1, :2], np.abs(c['X'][0, 0, 1:3, :, 0].astype(np.complex128))) and not want[0, 1, 2].any()
    assert np.array_equal(want[1, 2, :1], np.abs(c['z'][0][1, 0, 1:2].astype(np.complex128))) and not want[1, 2, 1:].any()
    assert np.array_equal(want[2, 2, :1], c['mask'][1, 0, 1:2]) and not want[2, 2, 1:].any()
