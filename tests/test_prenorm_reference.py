"""tests/prenorm_reference.py (the float reference the GPU suite uses for csrc/prenorm.hip) pinned to the fixture that
tests/golden/make_golden_prenorm.py produced with the reference's own data_gen/preprocess.py `pre_normalization`."""
import os

import numpy as np
import pytest

import prenorm_reference as R


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "prenorm_reference.npz"))


def test_restatement_equals_the_reference_bit_for_bit(gold):
    """same dtypes per step, same libm: any difference is a restatement bug"""
    x = gold["x"].copy()
    y = R.pre_normalization(x)
    assert y.dtype == np.float32 and y.shape == gold["y"].shape
    assert y.tobytes() == gold["y"].tobytes()
    assert x.tobytes() == gold["x"].tobytes()             # the input is left alone


def test_fixture_covers_what_it_claims(gold):
    x, y = gold["x"], gold["y"]
    assert x.shape == (4, 3, 120, 25, 2) and np.isfinite(y).all()
    frames = (x != 0).any(axis=(1, 3))                    # N, T, M
    assert not frames[1, :7, 0].any() and frames[1, 7, 0]                  # leading null frames
    assert frames[2, :60, 1].all() and not frames[2, 60:, 1].any()         # a second body of 60 frames
    assert not frames[[0, 1, 3], :, 1].any()
    assert all(0.2 <= a <= 2.9 for a in gold["angles"])
    angles = []
    R.pre_normalization(x, angles_out=angles)
    assert np.array_equal(np.asarray(angles).T.reshape(-1), gold["angles"])  # (z of every clip, then x of every clip)


def test_angle_between_docstring_values():
    """rotation.py:31-36"""
    assert R.angle_between((1, 0, 0), (0, 1, 0)) == 1.5707963267948966
    assert R.angle_between((1, 0, 0), (1, 0, 0)) == 0.0
    assert R.angle_between((1, 0, 0), (-1, 0, 0)) == 3.141592653589793


def test_identity_branches():
    """rotation.py:10 and :38: a bone on its axis and an antiparallel bone are both left alone"""
    for v in ((0, 0, 0.3), (0, 0, -0.3)):
        v = np.asarray(v, np.float32)
        assert np.array_equal(R.rotation_matrix(np.cross(v, [0, 0, 1]), R.angle_between(v, [0, 0, 1])), np.eye(3))
    assert R.angle_between(np.zeros(3, np.float32), [0, 0, 1]) == 0


def test_source_frames_closed_form():
    f = np.array([0, 0, 1, 0, 1, 1, 0, 0], bool)          # frame 0 null: compaction, L = 3, then the loop
    assert R.source_frames(f).tolist() == [2, 4, 5, 2, 4, 5, 2, 4]
    f = np.array([1, 0, 1, 0, 0, 0, 0, 0], bool)          # interior gap stays: L = 3 (frame 1 is still null after padding)
    assert R.source_frames(f).tolist() == [0, 1, 2, 0, 1, 2, 0, 1]
    f = np.array([1, 0, 0, 0, 0], bool)                   # L = 1
    assert R.source_frames(f).tolist() == [0, 0, 0, 0, 0]
    assert R.source_frames(np.zeros(4, bool)).tolist() == [0, 1, 2, 3]
