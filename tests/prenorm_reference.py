"""Float reference of the pre-normalisation (csrc/prenorm.hip): a numpy restatement of the reference's
data_gen/preprocess.py:8-88 `pre_normalization` and data_gen/rotation.py:5-42 with the SAME dtype at every step -- fp32
centring, fp32 bone and unit vector, float64 from the cross product on, `float64 matrix x fp32 joint` rounded to fp32 after
each of the two rotations.  The per-frame Python loops are replaced by array operations; the two 3 x 3 matrices are built per
clip with the reference's own numpy / math calls.  "Null" is ALL coordinates exactly zero (the reference tests sum() == 0: the
same unless coordinates cancel exactly).  Pinned bit for bit to a reference-produced fixture by tests/test_prenorm_reference.py;
the GPU suite compares the kernel against it where the reference itself is not available."""
import math

import numpy as np


def rotation_matrix(axis, theta):
    """rotation.py:5-20 -- Euler-Rodrigues; identity when sum|axis| < 1e-6 or |theta| < 1e-6"""
    if np.abs(axis).sum() < 1e-6 or np.abs(theta) < 1e-6:
        return np.eye(3)
    axis = np.asarray(axis)
    axis = axis / math.sqrt(np.dot(axis, axis))
    a = math.cos(theta / 2.0)
    b, c, d = -axis * math.sin(theta / 2.0)
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    bc, ad, ac, ab, bd, cd = b * c, a * d, a * c, a * b, b * d, c * d
    return np.array([[aa + bb - cc - dd, 2 * (bc + ad), 2 * (bd - ac)],
                     [2 * (bc - ad), aa + cc - bb - dd, 2 * (cd + ab)],
                     [2 * (bd + ac), 2 * (cd - ab), aa + dd - bb - cc]])


def angle_between(v1, v2):
    """rotation.py:28-42 -- 0 when either vector has sum|.| < 1e-6"""
    if np.abs(v1).sum() < 1e-6 or np.abs(v2).sum() < 1e-6:
        return 0
    v1_u = v1 / np.linalg.norm(v1)
    v2_u = v2 / np.linalg.norm(v2)
    return np.arccos(np.clip(np.dot(v1_u, v2_u), -1.0, 1.0))


def source_frames(frame_ok):
    """frame_ok (T,) bool of one body -> the source frame of every padded frame (preprocess.py:17-32 in closed form)"""
    T = len(frame_ok)
    t = np.arange(T)
    if not frame_ok.any():
        return t
    if not frame_ok[0]:                                   # compaction: the non-null frames move to the front in order
        keep = np.flatnonzero(frame_ok)
    else:                                                 # interior gaps stay where they are
        keep = np.arange(np.flatnonzero(frame_ok)[-1] + 1)
    L = len(keep)
    return keep[np.where(t < L, t, (t - L) % L)]


def _rotate(s, R, live):
    """s (M, T, V, 3) fp32 <- fp32(R (float64) @ joint) on the frames `live` (M, T); the others are left as they are"""
    p = s.astype(np.float64)
    # np.dot accumulates from +0: the leading 0.0 only keeps the sign of an all-zero joint's result (+0, not -0)
    r = np.stack([0.0 + R[i, 0] * p[..., 0] + R[i, 1] * p[..., 1] + R[i, 2] * p[..., 2] for i in range(3)], -1).astype(np.float32)
    return np.where(live[:, :, None, None], r, s)


def pre_normalization(data, zaxis=(0, 1), xaxis=(8, 4), angles_out=None):
    """(N, 3, T, V, M) fp32 -> a new array of the same shape; the input is not modified (the reference works in place).
    angles_out: a list that receives (theta_z, theta_x) of every clip (tests choose well-conditioned inputs with it)"""
    data = np.asarray(data)
    assert data.dtype == np.float32 and data.ndim == 5 and data.shape[1] == 3
    out = np.transpose(data, [0, 4, 2, 3, 1]).copy()      # N, M, T, V, C
    for n in range(out.shape[0]):
        s = out[n]
        body_ok = (s != 0).any(axis=(1, 2, 3))
        for m in np.flatnonzero(body_ok):                 # pad
            s[m] = s[m][source_frames((s[m] != 0).any(axis=(1, 2)))]
        if not body_ok.any():
            if angles_out is not None:
                angles_out.append((0.0, 0.0))
            continue
        thetas = []
        centre = s[0][:, 1:2, :].copy()                   # joint 1, hard-coded (preprocess.py:40)
        for m in np.flatnonzero(body_ok):
            mask = (s[m] != 0).any(axis=-1)[:, :, None]
            s[m] = (s[m] - centre) * mask
        for (j0, j1), target, sign in ((zaxis, [0, 0, 1], 1), (xaxis, [1, 0, 0], -1)):
            # z: joint_top - joint_bottom = s[z1] - s[z0]; x: joint_rshoulder - joint_lshoulder = s[x0] - s[x1]
            bone = s[0, 0, j1] - s[0, 0, j0] if sign > 0 else s[0, 0, j0] - s[0, 0, j1]
            theta = angle_between(bone, target)
            thetas.append(float(theta))
            R = rotation_matrix(np.cross(bone, target), theta)
            s[:] = _rotate(s, R, (s != 0).any(axis=(2, 3)))
        if angles_out is not None:
            angles_out.append(tuple(thetas))
    return np.transpose(out, [0, 4, 2, 3, 1]).copy()
