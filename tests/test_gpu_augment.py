"""csrc/augment.hip (sar_augment_clips_f32: temporal crop-resize + per-frame rotation, scale, shift of training clips) through
ops.augment_clips and sar_amd.augment.ClipAugment, against the float64 restatement tests/augment_reference.py.

Bar, per output coordinate:  |gpu - ref64| <= 8 * 2^-24 * (max(|near joint|, |far joint|) * s_max + d_max);  positions that are
exactly zero in the restatement must be exactly zero.  The 8 covers the fp32 roundings between the two: the blend (two products and
a sum), three products with fp32 matrix entries and their two sums, s and d rounded to fp32, the scale and the shift -- each at most
half a unit of a quantity bounded by |joint| s_max + d_max.  The float32 mode of the restatement (one rounding per operation, another
order than the kernel's fused multiply-adds) stays within 4 of these units (3.95 over the 120 000 joints of 8 clips of 300 frames,
profiles/augment.txt; the kernel: 3.02) at the maximum ranges rot = 0.3, scale = 0.1, shift = 0.2, crop = 0.5, which the
parameters here are drawn at.  When the kernel misses the bar, the float32 mode's own distance is printed next to it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_reference as A
from sar_amd.augment import NEUTRAL, ClipAugment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(rot=0.3, scale=0.1, shift=0.2, crop=0.5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gpu(x, tab, dev, crop=True):
    from sar_amd import ops
    y = ops.augment_clips(torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(tab)).to(dev), crop=crop)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def judge(got, x, tab, crop, what):
    """the worst coordinate's error in units of its bar; exact zeros compared exactly"""
    ref, bar = A.bound(x, tab, crop)
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    assert (got[ref == 0] == 0).all(), "%s: a position that is exactly zero in the restatement is not zero" % what
    live = ref != 0
    worst = float((np.abs(got.astype(np.float64) - ref)[live] / bar[live]).max() * 8) if live.any() else 0.0
    print("%s: max |gpu - ref64| = %.2f units of 2^-24 (|joint| s_max + d_max) (bar 8)" % (what, worst))
    if worst > 8:
        f32 = A.augment(x, tab, crop, "float32")
        print("%s: the float32 mode of the restatement: %.2f units" % (what, float((np.abs(f32.astype(np.float64) - ref)[live] / bar[live]).max() * 8)))
    assert worst <= 8, what
    return ref


# ------------------------------------------------------------------------------------------------ synthetic clips
def raw_clip(seed, T=37, V=25, M=2, edit=None):
    """(3, T, V, M): moving bodies somewhere in front of a camera, every joint non-null, then `edit`ed"""
    g = np.random.default_rng(seed)
    pose = g.normal(0, 0.3, (3, 1, V, M))
    walk = np.cumsum(g.normal(0, 0.01, (3, T, V, M)), axis=1)
    x = (pose + walk + g.uniform(-1, 1, (3, 1, 1, M)) + np.array([0, 0, 2.5]).reshape(3, 1, 1, 1)).astype(np.float32)
    assert (x != 0).all()
    if edit is not None:
        edit(x)
    return x


def drawn(n, seed):
    return ClipAugment(seed=seed, **FULL).table(n, 0, 0)


def _all_null(x):
    x[:] = 0


def _body1_null(x):
    x[..., 1] = 0


def _trailing(x):
    x[:, 20:] = 0


def _interior(x):
    x[:, 15] = 0


def _null_joint(x):
    x[:, 12, 7, 0] = 0
    x[:, 0, 3, 1] = 0


def _one_frame(x):
    x[:, 1:] = 0


def _with(**kw):
    def change(tab):
        for k, v in kw.items():
            tab[:, "po".index(k)] = v
    return change


# name -> (clip keywords, table edit): every clip is one batch of 1, the table drawn at the maximum ranges and then edited
CASES = {
    "plain": ({}, None),
    "every_body_null": ({"edit": _all_null}, None),
    "body1_null": ({"edit": _body1_null}, None),
    "trailing_padding_L20": ({"edit": _trailing}, None),
    "interior_null_frame_in_window": ({"edit": _interior}, _with(p=0.8, o=0.5)),          # L = 37, Lc = 29, b = 4: frame 15 is inside
    "null_joint_in_live_frame": ({"edit": _null_joint}, _with(p=1.0, o=0.0)),
    "L1": ({"edit": _one_frame}, None),
    "crop_to_Lc1": ({}, _with(p=0.01, o=0.4)),                                             # floor(0.37) = 0 -> Lc = 1, b = 14
    "o_rounds_to_one": ({}, _with(p=0.5, o=np.float32(0.99999999))),                       # b = min(19, 18)
    "T1": ({"T": 1}, None),
    "V32_M4": ({"T": 5, "V": 32, "M": 4}, None),
    "M1": ({"M": 1}, None),
    "T300": ({"T": 300}, None),
    "T515_two_record_chunks": ({"T": 515, "V": 7, "M": 1}, None),                          # AG_CHUNK = 512 frames per chunk
}
_cache = {}


def case(name):
    """(clip (1, 3, T, V, M), table (1, 16)) -- built once and never modified"""
    if name not in _cache:
        kw, change = CASES[name]
        k = sorted(CASES).index(name)
        x, tab = raw_clip(100 + k, **kw)[None], drawn(1, 100 + k)
        if change is not None:
            change(tab)
        x.setflags(write=False), tab.setflags(write=False)
        _cache[name] = (x, tab)
    return _cache[name]


def batch_of_8():
    names = ["plain", "every_body_null", "body1_null", "trailing_padding_L20", "interior_null_frame_in_window",
             "null_joint_in_live_frame", "L1", "crop_to_Lc1"]
    return np.concatenate([case(n)[0] for n in names]), np.concatenate([case(n)[1] for n in names])


# ------------------------------------------------------------------------------------------------ tests
def test_against_float64(dev):
    """8 clips, tables drawn at the maximum ranges, with and without the crop"""
    x = np.stack([raw_clip(s) for s in range(8)])
    x[5, :, 30:] = 0
    for seed in (0, 1):
        tab = drawn(8, seed)
        judge(gpu(x, tab, dev, True), x, tab, True, "drawn table %d, crop" % seed)
        judge(gpu(x, tab, dev, False), x, tab, False, "drawn table %d, no crop" % seed)


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_clips(dev, name):
    x, tab = case(name)
    got = gpu(x, tab, dev)
    ref = judge(got, x, tab, True, name)
    T = x.shape[2]
    if name == "every_body_null":
        assert not got.any()
    if name == "body1_null":
        assert not got[..., 1].any() and got[..., 0].all()
    if name == "trailing_padding_L20":
        assert got.all()                                       # the 20 valid frames are stretched over all 37
    if name == "interior_null_frame_in_window":
        b, Lc, i0, i1, frac = A.time_map(37, tab[0, 0], tab[0, 1], T)
        assert b <= 15 < b + Lc
        null_t = [t for t in range(T) if b + (i1[t] if frac[t] > 0.5 else i0[t]) == 15]
        assert null_t and all(not got[0, :, t].any() for t in null_t) and (ref == 0).all(axis=1).sum() == len(null_t) * 50
    if name == "null_joint_in_live_frame":
        assert not got[0, :, 12, 7, 0].any() and not got[0, :, 0, 3, 1].any() and got[0, :, 12, 7, 1].all()
    if name in ("L1", "crop_to_Lc1"):                          # one source frame: every output frame is a transform of it
        assert got.all()
        assert A.time_map(A.valid_length(x[0]), tab[0, 0], tab[0, 1], T)[1] == 1
    if name == "o_rounds_to_one":
        assert tab[0, 1] == 1.0 and A.time_map(37, tab[0, 0], tab[0, 1], T)[:2] == (19, 18)


def test_identity_is_bitwise(dev):
    x = np.stack([raw_clip(40), raw_clip(41, edit=_null_joint), raw_clip(42, edit=_interior)])
    tab = np.tile(NEUTRAL, (3, 1))
    assert gpu(x, tab, dev, True).tobytes() == x.tobytes()
    assert gpu(x, tab, dev, False).tobytes() == x.tobytes()
    padded = raw_clip(43, edit=_trailing)[None]                # crop off: the padding stays where it is
    assert gpu(padded, tab[:1], dev, False).tobytes() == padded.tobytes()
    big = raw_clip(44, T=300)[None]
    assert gpu(big, tab[:1], dev, True).tobytes() == big.tobytes()
    # the class with everything off is that identity
    from sar_amd.augment import ClipAugment
    y = ClipAugment()(torch.from_numpy(np.array(x)).to(dev), 3, 4)
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == x.tobytes()


def test_a_clip_does_not_depend_on_its_batch(dev):
    x, tab = batch_of_8()
    whole = gpu(x, tab, dev)
    for n in range(8):
        assert gpu(x[n:n + 1], tab[n:n + 1], dev).tobytes() == whole[n:n + 1].tobytes(), n


def test_two_runs_are_bitwise_equal(dev):
    x, tab = batch_of_8()
    assert gpu(x, tab, dev).tobytes() == gpu(x, tab, dev).tobytes()


def test_class_call_is_the_kernel_on_its_table(dev):
    """ClipAugment.__call__: the staged, asynchronously copied table gives what the table handed over directly gives, step after step"""
    aug = ClipAugment(seed=9, **FULL)
    x, _ = batch_of_8()
    xd = torch.from_numpy(x).to(dev)
    ys = [aug(xd, 2, it, rank=1) for it in range(4)]           # four steps in flight, no synchronisation between them
    torch.cuda.synchronize()
    for it, y in enumerate(ys):
        assert y.cpu().numpy().tobytes() == gpu(x, aug.table(8, 2, it, 1), dev).tobytes()
    assert ys[0].cpu().numpy().tobytes() != ys[1].cpu().numpy().tobytes()
    out = torch.empty_like(xd)
    assert aug(xd, 2, 0, rank=1, out=out) is out


def test_argument_errors_launch_nothing(dev, monkeypatch):
    from sar_amd import _lib as L, ops
    lib = L.load()
    x = torch.ones(2, 3, 5, 32, 2, device=dev)
    tab = torch.from_numpy(np.tile(NEUTRAL, (2, 1))).to(dev)
    out = torch.full_like(x, 7.0)

    def call(x, tab, out, N, T, V, M):
        rc = lib.sar_augment_clips_f32(x.data_ptr(), tab.data_ptr(), out.data_ptr(), N, T, V, M, 1, L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert call(x, tab, out, 2, 5, 33, 2) == L.SAR_E_UNSUP                      # V = 33
    assert call(x, tab, out, 2, 5, 32, 5) == L.SAR_E_UNSUP                      # M = 5
    assert call(x, tab, out, 1, 2049, 25, 2) == L.SAR_E_UNSUP                   # T = 2049 (rejected before anything is read)
    assert call(x, tab, out, 2, 0, 32, 2) == L.SAR_E_ARG
    assert call(x, tab, x, 2, 5, 32, 2) == L.SAR_E_ARG                          # out aliases x
    assert call(x, tab, x.view(-1)[3 * 5 * 32 * 2 - 8:], 1, 5, 32, 2) == L.SAR_E_ARG        # partial overlap
    assert call(x, out.view(-1)[16:], out, 2, 5, 32, 2) == L.SAR_E_ARG          # params inside out
    assert bool((out == 7.0).all()) and bool((x == 1.0).all())

    # the wrapper raises before the library is touched
    def forbidden():
        raise AssertionError("the library was loaded for a call with bad arguments")

    monkeypatch.setattr(L, "load", forbidden)
    bad = [
        lambda: ops.augment_clips(x[0], tab, out=out),                                           # not 5-D
        lambda: ops.augment_clips(x.double(), tab, out=out),                                     # not float32
        lambda: ops.augment_clips(x.cpu(), tab, out=out),                                        # not on the device
        lambda: ops.augment_clips(torch.ones(2, 4, 5, 32, 2, device=dev), tab),                  # C != 3
        lambda: ops.augment_clips(x, tab[:1], out=out),                                          # params of another length
        lambda: ops.augment_clips(x, tab[:, :15].contiguous(), out=out),
        lambda: ops.augment_clips(x, tab.double(), out=out),
        lambda: ops.augment_clips(x, tab.cpu(), out=out),
        lambda: ops.augment_clips(torch.ones(2, 3, 5, 33, 2, device=dev), tab),                  # over the limits
        lambda: ops.augment_clips(torch.ones(2, 3, 5, 8, 5, device=dev), tab),
        lambda: ops.augment_clips(torch.ones(1, 3, 2049, 2, 1, device=dev), tab[:1]),
        lambda: ops.augment_clips(x, tab, out=out[:, :, :, :25].contiguous()),                   # out of another shape
        lambda: ops.augment_clips(x, tab, out=x),                                                # out is x
        lambda: ops.augment_clips(x[:1], tab[:1], out=x.view(-1)[8:8 + x[0].numel()].view(x[:1].shape)),   # partial overlap
    ]
    for i, f in enumerate(bad):
        with pytest.raises((L.SarError, ValueError)):
            f()
            pytest.fail("argument error %d was accepted" % i)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((x == 1.0).all())


def test_cli_augment_trains(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "skeleton-action-recognition_amd"))
    cmd = [sys.executable, os.path.join(ROOT, "skeleton-action-recognition_amd", "main_gnn.py"), "--model", "stgcn", "--synthetic",
           "--synthetic-size", "16", "--batch-size", "4", "--max-iters", "3", "--augment", "rot=0.3,scale=0.1,shift=0.1,crop=0.5",
           "--num-epochs", "1", "--log-dir", str(tmp_path)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    runs = os.listdir(tmp_path)
    assert len(runs) == 1 and "augment:rot=0.3" in runs[0] and "augment_seed" not in runs[0]
    rows = [json.loads(line) for line in open(os.path.join(tmp_path, runs[0], "scalars.jsonl"))]
    losses = [r["value"] for r in rows if r["tag"] == "cross_entropy_loss"]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses), losses
    ck = torch.load(os.path.join(tmp_path, runs[0], "checkpoints", "ckpt-1.pt"), map_location="cpu")
    assert ck["iteration"] == 3 and bool(torch.isfinite(ck["velocity"]).all()) and bool(ck["velocity"].any())
    tensors = [v for v in ck["model"].values() if torch.is_tensor(v)]
    assert tensors and all(bool(torch.isfinite(v).all()) for v in tensors if v.is_floating_point())


def test_cli_without_the_flag_is_the_engine_alone(dev, tmp_path, monkeypatch):
    """flag off: the augmentation module is not imported, not one launch, the run name unchanged, and the first step's logits
    bitwise those of a direct call of a freshly built engine on the same batch"""
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
        raise AssertionError("augment_clips called without --augment")

    monkeypatch.setattr(Trainer, "step", recording_step)
    monkeypatch.setattr(ops, "augment_clips", forbidden)
    monkeypatch.delitem(sys.modules, "sar_amd.augment", raising=False)
    monkeypatch.setattr(sys, "argv", ["main_gnn.py", "--model", "stgcn", "--synthetic", "--synthetic-size", "16", "--max-iters", "1",
                                      "--num-epochs", "1", "--batch-size", "4", "--log-dir", str(tmp_path)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SAR_TRACE_DIR"):
        monkeypatch.delenv(k, raising=False)
    main_gnn.main()
    assert "sar_amd.augment" not in sys.modules
    runs = os.listdir(tmp_path)
    assert len(runs) == 1 and "augment" not in runs[0]
    x, y, logits = seen[0]
    from models.stgcn import Model
    eng = Model(num_classes=60, device=dev, stream="joint", mfma="fp32", trainable_adjacency=False).engine
    direct, _ = eng.loss_and_grad(x, y, x.shape[0])
    torch.cuda.synchronize()
    assert torch.equal(direct, logits)
