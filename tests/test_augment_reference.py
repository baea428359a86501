"""tests/augment_reference.py (the float64 restatement the GPU suite uses for csrc/augment.hip) against independent statements of
its parts -- torch's interpolate for the time map, scipy for the rotation -- and sar_amd/augment.py's parameter tables and parser.
No GPU."""
import numpy as np
import pytest
import torch

import augment_reference as A
from sar_amd.augment import NEUTRAL, ClipAugment

T = 37


def dense_clip(L, seed=0, V=5, M=2):
    """(3, T, V, M) float32: L frames without a null joint, then null padding"""
    g = np.random.default_rng(seed)
    x = np.zeros((3, T, V, M), dtype=np.float32)
    x[:, :L] = g.normal(0, 1, (3, L, V, M)).astype(np.float32) + np.float32(3)
    assert (x[:, :L] != 0).all()
    return x


def row(p=1.0, o=0.0, key0=(0, 0, 0, 1, 0, 0, 0), key1=None):
    return np.array([p, o, *key0, *(key0 if key1 is None else key1)], dtype=np.float32)


@pytest.mark.parametrize("L,p,o", [(37, 1, 0), (29, 0.6, 0.3), (5, 0.5, 1.0), (1, 0.7, 0.5), (37, 0.5, 0.999999)])
def test_resize_is_torch_linear_interpolation(L, p, o):
    x = dense_clip(L, seed=L)
    b, Lc, i0, i1, frac = A.time_map(L, np.float32(p), np.float32(o), T)
    assert Lc >= 1 and b >= 0 and b + Lc <= L and i1.max() <= Lc - 1
    if (L, p, o) == (5, 0.5, 1.0):
        assert (b, Lc) == (3, 2)                               # o = 1.0: floor(o (L - Lc + 1)) = 4 is cut back to L - Lc
    got = A.augment_clip(x, row(p, o), True, "float64", exact_weights=True)
    window = torch.from_numpy(x[:, b:b + Lc].astype(np.float64))           # (3, Lc, V, M) -> (1, 3 V M, Lc)
    want = torch.nn.functional.interpolate(window.permute(0, 2, 3, 1).reshape(1, -1, Lc), size=T, mode="linear", align_corners=False)
    want = want.reshape(3, x.shape[2], x.shape[3], T).permute(0, 3, 1, 2).numpy()
    err = np.abs(got - want).max()
    print("L %d p %g o %g: window [%d, %d), max |restatement - torch| = %.2e" % (L, p, o, b, b + Lc, err))
    assert err <= 1e-12
    # the contract's weight is float32(s - i0): the restatement proper differs from the exact-weight resize by that rounding alone
    proper = A.augment_clip(x, row(p, o), True, "float64")
    w = frac.astype(np.float32).astype(np.float64)[None, :, None, None]
    x0, x1 = x[:, b + i0].astype(np.float64), x[:, b + i1].astype(np.float64)
    assert np.array_equal(proper, (1 - w) * x0 + w * x1)


def test_full_length_window_has_zero_weights():
    b, Lc, i0, i1, frac = A.time_map(T, np.float32(1), np.float32(0), T)
    assert (b, Lc) == (0, T) and np.array_equal(i0, np.arange(T)) and not frac.any()


def test_rotation_is_scipy_extrinsic_xyz():
    from scipy.spatial.transform import Rotation
    g = np.random.default_rng(1)
    for a, b, c in np.vstack([g.uniform(-np.pi, np.pi, (50, 3)), np.zeros((1, 3)), [[0.3, -0.3, 0.3]]]):
        want = Rotation.from_euler("xyz", [a, b, c]).as_matrix()
        assert np.abs(A.rotation(a, b, c) - want).max() <= 1e-15
    assert np.array_equal(A.rotation(0.0, 0.0, 0.0), np.eye(3))


def test_parameters_move_linearly_between_the_key_frames():
    r = row(key0=(0.1, -0.2, 0.3, 0.9, 0.1, 0.2, -0.1), key1=(-0.3, 0.2, 0.1, 1.1, -0.2, 0.0, 0.2))
    R, s, d = A.frame_parameters(r, 5)
    r64 = r.astype(np.float64)
    assert R.dtype == np.float32 and np.array_equal(R[0], A.rotation(*r64[2:5]).astype(np.float32))
    assert np.array_equal(R[4], A.rotation(*r64[9:12]).astype(np.float32))
    assert s[0] == r64[5] and s[4] == r64[12] and np.array_equal(d[0], r64[6:9]) and np.array_equal(d[4], r64[13:16])
    assert abs(s[2] - 0.5 * (r64[5] + r64[12])) < 1e-15
    R1, s1, d1 = A.frame_parameters(r, 1)                     # T = 1: tau = 0, the start key frame
    assert np.array_equal(R1[0], R[0]) and s1[0] == s[0] and np.array_equal(d1[0], d[0])


@pytest.mark.parametrize("crop", [False, True])
def test_identity_is_bitwise_in_float32(crop):
    x = np.stack([dense_clip(T, seed=3), dense_clip(T, seed=4)])
    x[1, :, 5, 2, 0] = 0                                       # a null joint and an interior null frame stay what they are
    x[1, :, 9] = 0
    tab = np.stack([NEUTRAL, NEUTRAL])
    got = A.augment(x, tab, crop, "float32")
    assert got.dtype == np.float32 and got.tobytes() == x.tobytes()
    assert np.array_equal(A.augment(x, tab, crop, "float64"), x.astype(np.float64))
    padded = dense_clip(20)[None]                              # crop off keeps trailing padding; crop on stretches the 20 frames
    assert A.augment(padded, tab[:1], False, "float32").tobytes() == padded.tobytes()
    assert A.augment(padded, tab[:1], True, "float32")[0, :, 20:].all()


def test_null_rules():
    x = dense_clip(T, seed=5, V=3, M=1)
    x[:, 10] = 0                                               # interior null frame
    x[:, 20, 1] = 0                                            # a null joint in a live frame
    r = row(p=0.5, o=0.0, key0=(0.2, 0.1, -0.3, 1.1, 0.5, -0.5, 0.25))     # Lc = 18: output frames fall between source frames
    b, Lc, i0, i1, frac = A.time_map(T, r[0], r[1], T)
    terms = {}
    out = A.augment_clip(x, r, True, "float64", terms=terms)
    R, s, d = A.frame_parameters(r, T)
    seen = set()
    for t in range(T):
        near, far = (i1[t], i0[t]) if frac[t] > 0.5 else (i0[t], i1[t])
        near, far = b + near, b + far
        if near == 10:
            assert not out[:, t].any()                         # never a half-size blend, and no shift of a null joint
            seen.add("near")
        elif far == 10 and near != far:
            want = s[t] * (R[t].astype(np.float64) @ x[:, near].astype(np.float64).reshape(3, -1)) + d[t][:, None]
            assert np.allclose(out[:, t].reshape(3, -1), want, rtol=0, atol=1e-12)
            seen.add("far")
    assert seen == {"near", "far"}
    assert (out == 0).all(axis=0).sum() > 0 and terms["norm"].shape == (T, 3, 1)
    assert not A.augment_clip(np.zeros_like(x), r, True).any()                 # L = 0
    assert A.valid_length(x) == T and A.valid_length(np.zeros_like(x)) == 0


# ------------------------------------------------------------------------------------------------ ClipAugment.table
FULL = dict(rot=0.3, scale=0.1, shift=0.2, crop=0.5)


def test_table_is_a_function_of_its_key():
    aug = ClipAugment(seed=7, **FULL)
    a = aug.table(8, 3, 11, rank=2)
    assert a.dtype == np.float32 and a.shape == (8, 16)
    assert a.tobytes() == ClipAugment(seed=7, **FULL).table(8, 3, 11, rank=2).tobytes()
    assert a[:4].tobytes() == aug.table(4, 3, 11, rank=2).tobytes()            # a shorter batch is a prefix
    for other in (aug.table(8, 4, 11, 2), aug.table(8, 3, 12, 2), aug.table(8, 3, 11, 3), ClipAugment(seed=8, **FULL).table(8, 3, 11, 2)):
        assert not (other == a).all(axis=1).any() and (other != a).mean() > 0.99
    assert len({r.tobytes() for r in a}) == 8                                   # clips of one batch draw different rows


def test_every_draw_lies_inside_its_range():
    t = ClipAugment(seed=1, **FULL).table(4096, 0, 0)
    f = np.float32
    assert (t[:, 0] >= f(0.5)).all() and (t[:, 0] <= 1).all() and (t[:, 1] >= 0).all() and (t[:, 1] <= 1).all()
    for k in (2, 9):
        assert (np.abs(t[:, k:k + 3]) <= f(0.3)).all()
        assert (t[:, k + 3] >= f(0.9)).all() and (t[:, k + 3] <= f(1.1)).all()
        assert (np.abs(t[:, k + 4:k + 7]) <= f(0.2)).all()
    # ... and fills it: both halves of every range are reached
    assert t[:, 0].min() < 0.52 and t[:, 0].max() > 0.98 and t[:, 1].min() < 0.02 and t[:, 1].max() > 0.98
    assert t[:, 2:5].min() < -0.28 and t[:, 2:5].max() > 0.28 and t[:, 5].min() < 0.91 and t[:, 12].max() > 1.09
    assert (t[:, 2:9] != t[:, 9:16]).all()


def test_move_off_gives_equal_key_frames():
    t = ClipAugment(move=False, **FULL).table(64, 1, 2)
    assert np.array_equal(t[:, 2:9], t[:, 9:16]) and len(np.unique(t[:, 2])) == 64
    moving = ClipAugment(move=True, **FULL).table(64, 1, 2)
    assert np.array_equal(moving[:, :9], t[:, :9])             # the start key frame does not depend on `move`


def test_components_that_are_off_are_neutral():
    assert np.array_equal(ClipAugment().table(5, 2, 3), np.tile(NEUTRAL, (5, 1)))
    assert ClipAugment().table(5, 2, 3).tobytes() == np.tile(NEUTRAL, (5, 1)).tobytes()      # no negative zeros
    full = ClipAugment(**FULL).table(5, 2, 3)
    only_rot = ClipAugment(rot=0.3).table(5, 2, 3)
    want = np.tile(NEUTRAL, (5, 1))
    want[:, 2:5], want[:, 9:12] = full[:, 2:5], full[:, 9:12]                   # switching the others on does not move the angles
    assert np.array_equal(only_rot, want)
    only_crop = ClipAugment(crop=1.0).table(5, 2, 3)
    assert (only_crop[:, 0] == 1).all() and np.array_equal(only_crop[:, 1], full[:, 1])


def test_parser():
    a = ClipAugment.parse("rot=0.3,scale=0.1,shift=0.1,crop=0.5,move=1", seed=5)
    assert (a.rot, a.scale, a.shift, a.crop, a.move, a.seed) == (0.3, 0.1, 0.1, 0.5, True, 5)
    b = ClipAugment.parse("rot=0.2, move=0")
    assert (b.rot, b.scale, b.shift, b.crop, b.move, b.seed) == (0.2, 0.0, 0.0, None, False, 0)
    assert ClipAugment.parse("crop=1").crop == 1.0
    for bad in ("", "rot", "rot=", "rot=x", "spin=0.1", "rot=-0.1", "scale=-0.1", "scale=1", "shift=-1", "crop=0", "crop=1.5",
                "crop=-0.5", "move=2", "move=yes", "rot=0.1,rot=0.2", "rot=nan", "shift=inf", "rot=0.1,,scale=0.1"):
        with pytest.raises(ValueError):
            ClipAugment.parse(bad)
    with pytest.raises(ValueError):
        ClipAugment(crop=0.0)
    with pytest.raises(ValueError):
        ClipAugment(seed=-1)
