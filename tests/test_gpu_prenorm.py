"""csrc/prenorm.hip (sar_pre_normalize_f32: the reference's data_gen/preprocess.py `pre_normalization` on the device) through the C
ABI, against the reference-produced fixture tests/golden/prenorm_reference.npz and, at small synthetic shapes, against the numpy
restatement tests/prenorm_reference.py (pinned to that fixture bit for bit by tests/test_prenorm_reference.py).

Metric: max |gpu - ref| of a clip / that clip's max |coordinate|.  Bar 4e-6: each of the two rotations rounds once to fp32 (6e-8
relative); the angle carries the fp32 unit vector's error (<= ~2 ulp = 1.2e-7) amplified by 1 / sin(theta) <= 5 for bones between
0.2 and 2.9 rad from their axis (the fixture's generator asserts that; the synthetic clips are drawn until it holds); the device's
acos / sin / cos differ from the host's by ulps of double.  Positions that are exactly zero in the reference must be exactly zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prenorm_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 4e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gpu(x, dev, **kw):
    from sar_amd import ops
    y = ops.pre_normalize(torch.from_numpy(np.array(x)).to(dev), **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def judge(got, ref, what):
    """the worst clip's error; exact zeros compared exactly"""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert (got[ref == 0] == 0).all(), "%s: a position that is exactly zero in the reference is not zero" % what
    worst = 0.0
    for n in range(ref.shape[0]):
        scale = np.abs(ref[n]).max()
        err = np.abs(got[n].astype(np.float64) - ref[n]).max()
        worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else np.inf))
    print("%s: max |gpu - ref| / max |coordinate| = %.3e (bar %.1e)" % (what, worst, BAR))
    assert worst < BAR, what
    return worst


# ------------------------------------------------------------------------------------------------ synthetic raw clips
def raw_clip(seed, T, V=25, M=2, zaxis=(0, 1), xaxis=(8, 4), edit=None, exact=()):
    """(3, T, V, M): two moving bodies somewhere in front of a camera, every joint non-null, then `edit`ed; drawn again until both
    bones of body 0 are 0.2 .. 2.9 rad from their target axis (the condition the bar is derived under) -- except the bones listed
    in `exact` (0 = z, 1 = x), which the edit puts exactly on their axis or leaves null: the identity branches"""
    for attempt in range(1000):
        g = np.random.default_rng(seed * 1000 + attempt)
        pose = g.normal(0, 0.3, (3, 1, V, M))
        walk = np.cumsum(g.normal(0, 0.01, (3, T, V, M)), axis=1)
        x = (pose + walk + g.uniform(-1, 1, (3, 1, 1, M)) + np.array([0, 0, 2.5]).reshape(3, 1, 1, 1)).astype(np.float32)
        if edit is not None:
            edit(x, T)
        angles = []
        R.pre_normalization(x[None], zaxis, xaxis, angles_out=angles)
        if all(0.2 <= a <= 2.9 for i, a in enumerate(angles[0]) if i not in exact):
            return x
    raise AssertionError("no well-conditioned clip")


def _all_null(x, T):
    x[:] = 0


def _body1_null(x, T):
    x[..., 1] = 0


def _body0_null(x, T):
    x[..., 0] = 0


def _leading_null(x, T):
    x[:, :3, :, 0] = 0
    x[:, :1, :, 1] = 0


def _trailing_null(x, T):
    L = 7 if T >= 37 else 2                               # T - L is no multiple of L: 30 = 4 x 7 + 2, 57 = 8 x 7 + 1, 3 = 2 + 1
    assert (T - L) % L
    x[:, L:, :, 0] = 0
    x[:, 1:, :, 1] = 0                                    # L = 1


def _interior_gap(x, T):
    x[:, 2, :, 0] = 0                                     # valid frames follow: stays null
    if T >= 37:
        x[:, 10:15, :, 1] = 0
        x[:, 30:, :, 1] = 0                               # ... and is not taken for the end of the clip: L = 30


def _null_joint(x, T):
    x[:, 3, 7, 0] = 0
    x[:, 0, 12, 1] = 0


def _spine(sign):
    def make(x, T):                                       # hip -> spine exactly (0, 0, +-c) in frame 0
        x[:, 0, 0, 0] = x[:, 0, 1, 0]
        x[2, 0, 0, 0] -= np.float32(sign * 0.25)
    return make


def _shoulders(sign):
    def make(x, T):                                       # spine exactly +z (no z rotation), shoulders exactly (+-c, 0, 0)
        _spine(1)(x, T)
        x[:, 0, 8, 0] = x[:, 0, 4, 0]
        x[0, 0, 8, 0] += np.float32(sign * 0.375)
    return make


CASES = {
    "plain": (lambda x, T: None, {}),
    "all_null": (_all_null, {"exact": (0, 1)}),
    "body1_null": (_body1_null, {}),
    "body0_null": (_body0_null, {"exact": (0, 1)}),
    "leading_null_frames": (_leading_null, {}),
    "trailing_null_frames": (_trailing_null, {}),
    "interior_gap": (_interior_gap, {}),
    "null_joint": (_null_joint, {}),
    "spine_plus_z": (_spine(1), {"exact": (0,)}),
    "spine_minus_z": (_spine(-1), {"exact": (0,)}),
    "shoulders_plus_x": (_shoulders(1), {"exact": (0, 1)}),
    "shoulders_minus_x": (_shoulders(-1), {"exact": (0, 1)}),
    "other_axes": (lambda x, T: None, {"zaxis": (2, 3), "xaxis": (5, 9)}),
    "kinetics_v18": (lambda x, T: None, {"V": 18}),
}
_cache = {}


def case(name, T):
    """(raw clip (1, 3, T, V, M), reference output, axes) -- built once per (case, T) and never modified"""
    if (name, T) not in _cache:
        edit, opt = CASES[name]
        axes = {k: opt[k] for k in ("zaxis", "xaxis") if k in opt}
        x = raw_clip(sorted(CASES).index(name) * 100 + T, T, V=opt.get("V", 25), edit=edit, exact=opt.get("exact", ()), **axes)[None]
        ref = R.pre_normalization(x, **axes)
        x.setflags(write=False), ref.setflags(write=False)
        _cache[name, T] = (x, ref, axes)
    return _cache[name, T]


def centred_only(x):
    """padding and centring without any rotation, for clips that need no padding: (x - body 0's joint 1) * joint mask, in fp32"""
    s = np.transpose(x, [0, 4, 2, 3, 1])
    out = (s - s[:, :1, :, 1:2, :]) * (s != 0).any(axis=-1, keepdims=True)
    return np.transpose(out, [0, 4, 2, 3, 1])


@pytest.mark.parametrize("T", [5, 37, 64])
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(dev, name, T):
    x, ref, axes = case(name, T)
    got = gpu(x, dev, **axes)
    judge(got, ref, "%s T=%d" % (name, T))
    if name == "all_null":
        assert not got.any()
    if name == "body0_null":                              # centre 0, identity rotations: body 1 passes through
        assert np.array_equal(got, x)
    if name == "interior_gap":
        assert not got[0, :, 2, :, 0].any() and got[0, :, 3, :, 0].any()
    if name == "null_joint":
        assert not got[0, :, 3, 7, 0].any() and not got[0, :, 0, 12, 1].any()
    if name == "trailing_null_frames":
        L = 7 if T >= 37 else 2
        assert np.array_equal(got[0, :, L:2 * L, :, 0][:, :min(L, T - L)], got[0, :, :min(L, T - L), :, 0])
    if name.startswith("spine"):
        # identity for the z rotation in BOTH directions: bitwise what zaxis = (0, 0) (a zero bone, no z rotation) gives
        assert np.array_equal(ref, R.pre_normalization(x, zaxis=(0, 0)))
        assert got.tobytes() == gpu(x, dev, zaxis=(0, 0)).tobytes()
    if name.startswith("shoulders"):
        assert np.array_equal(got, ref) and np.array_equal(got, centred_only(x))   # two identities: bit-equal to centring alone


def test_against_the_reference_fixture(dev, golden_dir):
    gold = np.load(os.path.join(golden_dir, "prenorm_reference.npz"))
    worst = judge(gpu(gold["x"], dev), gold["y"], "golden (4 clips, T = 120)")
    print("PRENORM_GOLDEN_WORST %.3e" % worst)


def batch_of_8(T=37):
    names = ["plain", "leading_null_frames", "trailing_null_frames", "interior_gap", "null_joint", "body0_null", "all_null",
             "spine_minus_z"]
    return np.concatenate([case(n, T)[0] for n in names])


def test_a_clip_does_not_depend_on_its_batch(dev):
    x = batch_of_8()
    whole = gpu(x, dev)
    for n in range(8):
        assert gpu(x[n:n + 1], dev).tobytes() == whole[n:n + 1].tobytes(), n


def test_two_runs_are_bitwise_equal(dev):
    x = batch_of_8(64)
    assert gpu(x, dev).tobytes() == gpu(x, dev).tobytes()


def test_argument_errors_launch_nothing(dev):
    from sar_amd import _lib as L, ops
    lib = L.load()

    def call(x, out, N, T, V, M, z0=0, z1=1, x0=8, x1=4):
        rc = lib.sar_pre_normalize_f32(x.data_ptr(), out.data_ptr(), N, T, V, M, z0, z1, x0, x1, L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    x = torch.ones(2, 3, 5, 33, 2, device=dev)
    out = torch.full_like(x, 7.0)
    assert call(x, out, 2, 5, 33, 2) == L.SAR_E_UNSUP                      # V = 33
    assert call(x, out, 2, 5, 32, 2, x0=32) == L.SAR_E_ARG                 # joint index >= V
    assert call(x, out, 2, 5, 32, 2, z1=-1) == L.SAR_E_ARG
    assert call(x, out, 2, 5, 32, 5) == L.SAR_E_UNSUP                      # M = 5
    assert call(x, out, 1, 2049, 25, 2) == L.SAR_E_UNSUP                   # T = 2049 (rejected before anything is read)
    assert call(x, x, 2, 5, 32, 2) == L.SAR_E_ARG                          # out aliases x
    assert call(x, x.view(-1)[3 * 5 * 32 * 2 - 8:], 1, 5, 32, 2) == L.SAR_E_ARG   # partial overlap
    assert bool((out == 7.0).all()) and bool((x == 1.0).all())
    with pytest.raises(L.SarError):
        ops.pre_normalize(torch.ones(2, 4, 5, 25, 2, device=dev))          # C != 3
    with pytest.raises(L.SarError):
        ops.pre_normalize(x[:, :, :, :32].contiguous(), out=out)           # out of another shape
    with pytest.raises(L.SarError):
        y = x[:, :, :, :25].contiguous()
        ops.pre_normalize(y, out=y)


def test_numpy_input_goes_through_the_device_in_chunks(dev, monkeypatch, tmp_path):
    from data_gen import preprocess
    from data_gen.preprocess import pre_normalization
    x = np.concatenate([batch_of_8()[:4], case("plain", 37)[0]])           # 5 clips, chunks of 2 + 2 + 1
    monkeypatch.setattr(preprocess, "CHUNK", 2)
    got = pre_normalization(x)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    t = pre_normalization(torch.from_numpy(x).to(dev))
    assert t.is_cuda and got.tobytes() == t.cpu().numpy().tobytes()
    assert got.tobytes() == gpu(x, dev).tobytes()
    mm = np.lib.format.open_memmap(str(tmp_path / "raw.npy"), mode="w+", dtype=np.float32, shape=x.shape)
    mm[:] = x
    assert pre_normalization(mm).tobytes() == got.tobytes()


def test_cli_pre_normalize_trains(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "skeleton-action-recognition_amd"))
    cmd = [sys.executable, os.path.join(ROOT, "skeleton-action-recognition_amd", "main_gnn.py"), "--model", "stgcn", "--synthetic",
           "--synthetic-size", "16", "--pre-normalize", "--max-iters", "2", "--num-epochs", "1", "--batch-size", "4",
           "--log-dir", str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    runs = os.listdir(tmp_path)
    assert len(runs) == 1 and "pre_normalize:True" in runs[0]
    rows = [json.loads(line) for line in open(os.path.join(tmp_path, runs[0], "scalars.jsonl"))]
    losses = [r["value"] for r in rows if r["tag"] == "cross_entropy_loss"]
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses), losses


def test_cli_without_the_flag_is_the_engine_alone(dev, tmp_path, monkeypatch):
    """flag off: not one pre-normalisation launch, the run name unchanged, and the first step's logits bitwise those of a direct
    call of a freshly built engine on the same batch"""
    import main_gnn
    from sar_amd import ops
    from sar_amd.train import Trainer
    seen = []
    step = Trainer.step

    def recording_step(self, x, y):
        logits, loss = step(self, x, y)
        if not seen:
            seen.append((x.clone(), y.clone(), logits.clone()))
        return logits, loss

    def forbidden(*a, **k):
        raise AssertionError("pre_normalize called without --pre-normalize")

    monkeypatch.setattr(Trainer, "step", recording_step)
    monkeypatch.setattr(ops, "pre_normalize", forbidden)
    monkeypatch.setattr(sys, "argv", ["main_gnn.py", "--model", "stgcn", "--synthetic", "--synthetic-size", "16", "--max-iters", "1",
                                      "--num-epochs", "1", "--batch-size", "4", "--log-dir", str(tmp_path)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAR_TRACE_DIR"):
        monkeypatch.delenv(k, raising=False)
    main_gnn.main()
    runs = os.listdir(tmp_path)
    assert len(runs) == 1 and "pre_normalize" not in runs[0]
    x, y, logits = seen[0]
    from models.stgcn import Model
    eng = Model(num_classes=60, device=dev, stream="joint", mfma="fp32", trainable_adjacency=False).engine
    direct, _ = eng.loss_and_grad(x, y, x.shape[0])
    torch.cuda.synchronize()
    assert torch.equal(direct, logits)
