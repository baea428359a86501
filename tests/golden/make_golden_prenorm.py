"""Writes tests/golden/prenorm_reference.npz: raw (un-normalised) clips and what the reference's
data_gen/preprocess.py `pre_normalization` (imported from the reference checkout, not copied) makes of them.

Inputs: the reference's four bundled clips (data/NTU_preprocessed_skeleton_examples.npy) cropped to 120 frames and un-normalised
by a rigid rotation of about 0.7 rad about y plus a translation (null joints stay null); clip 1 gets 7 leading null frames,
clip 2 a second body that lasts 60 frames.  Asserted here: `sum() == 0` (the reference's null test) and `all == 0` (the kernel's)
agree on every body, frame and joint of the inputs, and both bones make an angle in [0.2, 2.9] rad with their target axis, so
that arccos is well conditioned.  (Joint 1 is null in frame 0 of every bundled clip and stays null, so the centre of that frame is
0 and the hip -> spine bone of a clip without leading null frames is minus the hip's raw position: the translations are mostly
sideways, not along z, to keep that bone away from -z.)

    SAR_REFERENCE=<reference checkout> python tests/golden/make_golden_prenorm.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SAR_REFERENCE") or os.path.join(HERE, "..", "..", "..", "reference")   # default: a checkout beside this one
T = 120

try:
    import tqdm  # noqa: F401
except ImportError:                                       # the reference only wraps its loops in it
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, *a, **k: it)
sys.path.insert(0, REF)
from data_gen import preprocess as P                       # noqa: E402


def y_rotation(theta):
    c, s = np.float32(np.cos(theta)), np.float32(np.sin(theta))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)


def unnormalise(body, theta, shift):
    """body (3, T, V) fp32 -> rotated about y and translated, null joints kept null"""
    live = (body != 0).any(axis=0, keepdims=True)
    moved = np.einsum("ij,jtv->itv", y_rotation(theta), body) + np.asarray(shift, np.float32)[:, None, None]
    return np.where(live, moved, 0).astype(np.float32)


clips = np.load(os.path.join(REF, "data", "NTU_preprocessed_skeleton_examples.npy"))[:, :, :T].astype(np.float32)
x = np.zeros_like(clips)
for n in range(4):
    x[n, :, :, :, 0] = unnormalise(clips[n, :, :, :, 0], 0.7 + 0.05 * n, (0.9 - 0.1 * n, 0.5 + 0.05 * n, 0.7 + 0.1 * n))
x[1, :, :7] = 0                                           # leading null frames: compaction
second = clips[2, :, np.arange(60) % 50, :, 0].transpose(1, 0, 2)        # clip 2 has 50 frames; the second body lasts 60
x[2, :, :60, :, 1] = unnormalise(second, 0.55, (-0.4, 0.25, 1.1))

# the two null tests agree on every body, frame and joint
s = x.transpose(0, 4, 2, 3, 1)                            # N, M, T, V, C
for axes in ((2, 3, 4), (3, 4), (4,)):
    assert np.array_equal(s.sum(axis=axes) == 0, (s == 0).all(axis=axes)), axes

angles = []
_rotation_matrix = P.rotation_matrix


def recording(axis, theta):
    angles.append(float(theta))
    return _rotation_matrix(axis, theta)


P.rotation_matrix = recording
with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
    y = np.ascontiguousarray(P.pre_normalization(x.copy()))     # the reference works in place
assert len(angles) == 8 and all(0.2 <= a <= 2.9 for a in angles), angles
assert y.dtype == np.float32 and np.isfinite(y).all()
print("angles (z then x, per clip):", ["%.3f" % a for a in angles], "max |coordinate| %.3f" % np.abs(y).max())
path = os.path.join(HERE, "prenorm_reference.npz")
np.savez_compressed(path, x=x, y=y, angles=np.asarray(angles))
print(path, os.path.getsize(path), "bytes")
