"""GPU: d loss / d clip of the ST-GCN engines -- the backward apply pass of data_bn (include/sar_hip.h: sar_data_bn_bwd_apply_f32 /
_cn8), `need_dx` of the engines, and `x.grad` through models.stgcn.Model.

Kernel level, both variants, against the float64 restatement tests/data_bn_dx_reference.py with random dh and random k1..k3:

    |got - ref| <= 16 * 2^-24 * S        per element, S = the sum of |k1 dh| + |k2 val| + |k3| over the dvals that reach the element

derived, not measured: at most 12 dvals reach one output (own term and the 5 children of the NTU root -- or of any joint: the root
forms no own term --, times 2 for motion); each dval is two fused roundings, a motion difference one more per joint (6), the children
5 more: 2 + 6 + 5 = 13 roundings, each at most 2^-24 of a partial sum that S bounds; 16 leaves room for another order.  The kernel
adds the terms in exactly that order (csrc/elementwise.hip: data_bn_bwd_apply_kernel), so the constant stays 16.  bf16 -> float32 is
exact, so the CN8 variant has the same bound with dh drawn as bf16.  Exact results: motion at T = 1 is all +0 bits; a self-pair
contributes exactly nothing (dx of a childless self-pair is +0, dx does not depend on the dh that arrives at the NTU root); two runs
are bitwise equal.

Engine level: dx of loss_and_grad(..., need_dx=True) against torch.autograd.grad of the float64 oracle with respect to x, the oracle
conditioned on the engine's ReLU masks, at TOL = 1e-4 (max-norm relative) like every other gradient tensor.  The float32-oracle-vs-
float64-oracle band of dx at these shapes (computed on a CPU, unconditioned, streams joint / bone_motion):
    two blocks (2,3,12,25,2)  2.8e-07 / 4.0e-07        ragged (1,3,4,25,1)  8.9e-07 / 1.5e-06        ragged (5,3,33,25,3)  7.8e-07 / 6.6e-07
all far below 2.5e-5, so max(4 * band, TOL) is TOL.  (tests/test_gpu_stgcn_model.py's ragged shapes hold no case that is both single
body and odd T: (1, 4, 1) is the single-body one, (5, 33, 3) the odd-T one; both run.)

bf16 engine (the configuration of tests/test_gpu_bf16.py::test_train_step_bf16_close_to_fp32): cos(dx_bf16, dx_fp32) > 0.98, the
project's bound for that configuration; the cosine of data_bn.gamma's gradient -- same depth -- is printed beside it (measured on
an MI355X: cos(dx) = 0.98387, cos(d data_bn.gamma) = 0.98504)."""
import functools

import pytest
import torch

import data_bn_dx_reference as R
from oracle import stgcn as O
from util import (NAN, SENTINEL, _bits, assert_flat_guards_untouched, cn8_units, guarded, guarded_cn8, guarded_flat, rel_err)

pytestmark = pytest.mark.gpu
TOL = 1e-4
BOUND = 16 * 2.0 ** -24
STREAMS = list(R.STREAMS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _frames():
    from sar_amd import ops
    return ops.DATA_BN_DX_FRAMES


def _shapes():
    return [(1, 3, 1, 25, 1), (2, 3, 2, 25, 2), (2, 3, _frames() + 1, 25, 2), (3, 1, 7, 5, 3), (2, 8, 19, 25, 2)]


def _parent(stream, V):
    if not R.STREAMS[stream][0]:
        return None
    return R.ntu_parent() if V == 25 else R.HAND_PARENT


@functools.lru_cache(maxsize=None)
def _case(shape, stream, bf16):
    """host operands of one kernel-level case and its float64 reference: computed once, shared, never modified"""
    N, C, T, V, M = shape
    g = torch.Generator().manual_seed(sum(s * 31 ** i for i, s in enumerate(shape)) + STREAMS.index(stream) + 7 * bf16)
    x = torch.randn(shape, generator=g)
    dh = torch.randn(C, N * M * T * V, generator=g)
    if bf16:
        dh = dh.bfloat16().float()
    k = tuple(torch.randn(V * C, generator=g) for _ in range(3))
    parent, motion = _parent(stream, V), R.STREAMS[stream][1]
    ref, S = R.data_bn_dx(x, dh, *k, parent, motion)
    return dict(x=x, dh=dh, k=k, parent=parent, motion=motion, ref=ref, S=S)


def _run(dev, c, variant, dh=None, pad=None, dx=None):
    """one launch.  pad: dh as a view into a larger allocation (ld = n + pad, NaN all around); dx: the output to write"""
    from sar_amd import ops, ops8
    dh = c["dh"] if dh is None else dh
    parent = None if c["parent"] is None else torch.from_numpy(c["parent"]).to(dev)
    k = tuple(t.to(dev) for t in c["k"])
    x = c["x"].to(dev)
    if variant == "cn8":
        dy = cn8_units(dh).to(dev) if pad is None else guarded_cn8(dh, pad, NAN, dev)[0]
        out = ops8.data_bn_bwd_apply(x, parent, dy, k, dx=dx, motion=c["motion"])
    else:
        dy = dh.to(dev) if pad is None else guarded(dh, pad, NAN, dev)[0]
        out = ops.data_bn_bwd_apply(x, parent, dy, k, dx=dx, motion=c["motion"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("variant", ["f32", "cn8"])
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("si", range(5))
def test_kernel_against_float64(dev, si, stream, variant):
    shape = _shapes()[si]
    N, C, T, V, M = shape
    c = _case(shape, stream, variant == "cn8")
    got = _run(dev, c, variant).cpu()
    again = _run(dev, c, variant).cpu()
    assert torch.equal(_bits(got), _bits(again)), "two runs differ"
    err = (got.double() - c["ref"]).abs()
    ratio = (err / c["S"].clamp(min=1e-300)).max().item()
    print("%s %s %s: worst |got - ref| / S = %.2f * 2^-24" % (shape, stream, variant, ratio * 2 ** 24))
    assert torch.isfinite(got).all()
    assert (err <= BOUND * c["S"]).all(), "worst |got - ref| / S = %.3e > %.3e" % (ratio, BOUND)
    if c["motion"] and T == 1:
        assert bool((_bits(got) == 0).all()), "motion at T = 1: dx must be all +0"
    if c["parent"] is not None and V == 5:
        assert bool((_bits(got[:, :, :, 4].contiguous()) == 0).all()), "a childless self-pair: dx must be +0"
    if c["parent"] is not None and V == 25:
        # what arrives at the root (a self-pair with four children) reaches no element of dx
        clip = R.cn_to_clip(c["dh"], N, C, T, V, M).clone()
        clip[:, :, :, 20] = 3.0
        other = _run(dev, c, variant, dh=R.clip_to_cn(clip).contiguous()).cpu()
        assert torch.equal(_bits(got), _bits(other)), "dx depends on the gradient arriving at the root self-pair"


@pytest.mark.parametrize("variant", ["f32", "cn8"])
@pytest.mark.parametrize("stream", ["joint", "bone_motion"])
@pytest.mark.parametrize("si", [2, 3])
def test_guard_bands(dev, si, stream, variant):
    """dh with a padded leading dimension and NaN in the margins, dx between poisoned guards -- the guards stay intact,
    the bits equal the tight run's, no NaN reaches dx; a leading dimension below the live width is rejected and writes nothing"""
    from sar_amd._lib import SarError
    shape = _shapes()[si]
    c = _case(shape, stream, variant == "cn8")
    tight = _run(dev, c, variant)
    n = c["x"].numel()
    for pad in (1, 67):
        view, whole = guarded_flat(n, SENTINEL, dev)
        got = _run(dev, c, variant, pad=pad, dx=view.view(shape))
        assert got.data_ptr() == view.data_ptr()
        assert_flat_guards_untouched(whole, n, SENTINEL, what="dx, pad %d" % pad)
        assert torch.isfinite(got).all()
        assert torch.equal(_bits(got), _bits(tight)), "pad %d: the bits differ from the tight run's" % pad
    view, whole = guarded_flat(n, SENTINEL, dev)
    short = c["dh"][:, :-1].clone()
    with pytest.raises(SarError, match="sar_data_bn_bwd_apply_" + variant):
        _run(dev, c, variant, dh=short, dx=view.view(shape))
    assert bool((whole == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ engines
def _oracle_dx(forward, p, x, y, blocks, masks, parent, motion, dtype=torch.float64):
    """d loss / d x of a float64 restatement `forward` fed the stream's values of x"""
    xr = x.to(dtype).clone().requires_grad_(True)
    q = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    logits = forward(q, R.stream_values(xr, parent, motion), True, {}, {}, blocks, masks)
    return torch.autograd.grad(O.loss_fn(logits, y, x.shape[0]), xr)[0]


def _engine_dx_case(dev, make_engine, forward, masks_of, p, x, y, blocks, stream="joint"):
    """need_dx=True against the conditioned float64 oracle; every parameter gradient bitwise that of a need_dx=False step"""
    bone, motion = R.STREAMS[stream]
    eng = make_engine()
    assert eng.motion == motion and (eng.bone_parent is not None) == bone
    eng.load_params(p)
    keep = {}
    xg, yg = x.to(dev), y.to(dev)
    eng.forward(xg, training=True, keep=keep)
    masks = masks_of(eng, keep, blocks, x.shape[0] * x.shape[4], x.shape[2])
    ref = _oracle_dx(forward, p, x, y, blocks, masks, R.ntu_parent() if bone else None, motion)
    eng.load_params(p)
    out = eng.loss_and_grad(xg, yg, need_dx=True)
    torch.cuda.synchronize()
    assert len(out) == 3
    logits, loss, dx = out
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous()
    grad = eng.grad.clone()
    eng.load_params(p)
    out2 = eng.loss_and_grad(xg, yg)
    torch.cuda.synchronize()
    assert len(out2) == 2 and torch.equal(out2[0], logits) and torch.equal(out2[1], loss)
    assert torch.equal(_bits(eng.grad), _bits(grad)), "need_dx changed a parameter gradient"
    e = rel_err(dx.cpu(), ref)
    print("dx vs the conditioned float64 oracle: %.3e (max|dx| %.3e)" % (e, ref.abs().max().item()))
    assert ref.abs().max().item() > 0 and e < TOL
    return eng, dx


TWO = [(64, 1, False), (64, 1, True)]
THREE = [(64, 1, False), (64, 1, True), (128, 2, True)]


def _stgcn_case(which):
    """(blocks, p, x, y) of tests/test_gpu_stgcn_model.py: test_two_blocks_small and test_tiny_and_ragged_shapes"""
    if which == "two":
        blocks, N, T, M, classes, seed, xseed = TWO, 2, 12, 2, 10, 0, 0
    else:
        N, T, M = which
        blocks, classes, seed, xseed = THREE, 7, 21, 20 + T
    p = O.randomize_affine(O.init_params(classes, seed=seed, dtype=torch.float64, blocks=blocks), seed=seed + 1)
    x, y = O.synthetic_batch(N, seed=xseed, T=T, M=M, num_classes=classes)
    return blocks, p, x, y


@pytest.mark.parametrize("mfma", ["fp32", "f32_split"])
@pytest.mark.parametrize("stream", ["joint", "bone_motion"])
@pytest.mark.parametrize("which", ["two", (1, 4, 1), (5, 33, 3)])
def test_stgcn_engine_dx(dev, which, stream, mfma):
    from sar_amd.bone import NTU_BONE_PAIRS
    from sar_amd.stgcn import STGCN
    from test_gpu_stgcn_model import _engine_masks
    blocks, p, x, y = _stgcn_case(which)
    bone, motion = R.STREAMS[stream]
    make = lambda: STGCN(num_classes=p["logits.bias"].numel(), device=dev, blocks=blocks, mfma=mfma,
                         bone_pairs=NTU_BONE_PAIRS if bone else None, motion=motion)
    _engine_dx_case(dev, make, O.forward, _engine_masks, p, x, y, blocks, stream)


def test_backward_without_a_training_forward_still_raises(dev):
    from sar_amd.stgcn import STGCN
    eng = STGCN(num_classes=10, device=dev, blocks=TWO)
    x, _ = O.synthetic_batch(2, seed=0, T=12, num_classes=10)
    eng.forward(x.to(dev), training=False)
    with pytest.raises(AssertionError, match="training=True"):
        eng.backward(torch.ones(2, 10, device=dev), need_dx=True)


def test_stgin_engine_dx(dev):
    from oracle import stgin as G
    from sar_amd.stgin import STGIN
    from test_gpu_stgin import _engine_masks, _params
    p = _params(TWO, 10, 0)
    x, y = O.synthetic_batch(2, seed=0, T=12, num_classes=10)
    _engine_dx_case(dev, lambda: STGIN(num_classes=10, device=dev, blocks=TWO), G.forward, _engine_masks, p, x, y, TWO)


def test_stpgcn_engine_dx(dev):
    import pgc_reference as P
    from sar_amd.stpgcn import STPGCN
    from test_gpu_stpgcn import _masks, _params
    p = _params(TWO, 10, 0)
    x, y = O.synthetic_batch(2, seed=0, T=12, num_classes=10)
    _engine_dx_case(dev, lambda: STPGCN(num_classes=10, device=dev, blocks=TWO), P.forward, _masks, p, x, y, TWO)


def test_stgcn_ta_engine_dx(dev):
    import stgcn_ta_reference as A
    from sar_amd.stgcn_ta import STGCNTA
    from test_gpu_stgcn_model import _engine_masks
    from test_gpu_stgcn_ta import _params, _perturbed_tables
    p = _perturbed_tables(_params(TWO, 10, 2), 12, TWO, 5)
    x, y = O.synthetic_batch(2, seed=4, T=12, num_classes=10)
    _engine_dx_case(dev, lambda: STGCNTA(num_classes=10, device=dev, blocks=TWO, frames=12), A.forward, _engine_masks, p, x, y, TWO)


def test_bf16_engine_dx_points_the_fp32_way(dev):
    from sar_amd.stgcn import STGCN
    blocks = [(64, 1, False), (64, 1, True), (128, 2, True), (128, 1, True)]
    p = O.randomize_affine(O.init_params(10, seed=0, dtype=torch.float64, blocks=blocks))
    x, y = O.synthetic_batch(4, seed=0, T=40, num_classes=10)
    out = {}
    for mode in ("fp32", "bf16"):
        eng = STGCN(num_classes=10, device=dev, blocks=blocks, mfma=mode)
        eng.load_params(p)
        _, _, dx = eng.loss_and_grad(x.to(dev), y.to(dev), need_dx=True)
        torch.cuda.synchronize()
        out[mode] = (dx.cpu().double(), eng.g["data_bn.gamma"].cpu().double().clone())
    cos = lambda a, b: ((a * b).sum() / (a.norm() * b.norm())).item()
    cos_dx, cos_gamma = cos(out["fp32"][0], out["bf16"][0]), cos(out["fp32"][1], out["bf16"][1])
    print("bf16 vs fp32 engine: cos(dx) = %.5f, cos(d data_bn.gamma) = %.5f" % (cos_dx, cos_gamma))
    assert torch.isfinite(out["bf16"][0]).all()
    assert cos_dx > 0.98


# ------------------------------------------------------------------------------------------------ autograd
@pytest.fixture()
def launches(monkeypatch):
    """counts the data_bn_bwd_apply launches of the fp32 engines"""
    from sar_amd import ops
    count, real = [0], ops.data_bn_bwd_apply

    def counted(*a, **kw):
        count[0] += 1
        return real(*a, **kw)
    monkeypatch.setattr(ops, "data_bn_bwd_apply", counted)
    return count


def test_model_fills_x_grad(dev, launches):
    from models.stgcn import Model
    model = Model(num_classes=10, device=dev, seed=1, stream="bone_motion", blocks=TWO)
    x, _ = O.synthetic_batch(2, seed=1, T=12, num_classes=10)
    xg = x.to(dev)
    model(xg, True).sum().backward()                       # x asks for nothing: no launch, the parameters get theirs
    assert launches[0] == 0 and xg.grad is None
    assert model.data_bn_gamma.grad is not None
    xr = xg.clone().requires_grad_(True)
    model(xr, True).sum().backward()
    assert launches[0] == 1
    eng = model.engine
    logits = eng.forward(xg, training=True)
    dx = eng.backward(torch.ones_like(logits), need_dx=True)
    torch.cuda.synchronize()
    assert xr.grad is not None and xr.grad.abs().max().item() > 0
    assert torch.equal(_bits(xr.grad), _bits(dx))


def test_sampler_in_front_of_the_model_trains_its_scorer(dev):
    """TemporalSampler -> models.stgcn.Model: before the engines had an input gradient the scorer's gradients were None"""
    from models.lstm_sampler import TemporalSampler
    from models.stgcn import Model
    N, C, T, V, M, k = 2, 3, 10, 25, 2, 6
    torch.manual_seed(0)
    sampler = TemporalSampler([8], top_k=k)
    model = Model(num_classes=10, device=dev, seed=2, blocks=TWO)
    x, y = O.synthetic_batch(N, seed=5, T=T, num_classes=10)
    picked = sampler(x.to(dev).reshape(N, C, T, V * M), True)              # (N, C, k, V M): a non-leaf input of the model
    clip = picked.view(N, C, k, V, M)
    clip.retain_grad()
    logits = model(clip, True)
    loss = torch.nn.functional.cross_entropy(logits, y.to(dev), reduction="sum") / N
    dlogits, = torch.autograd.grad(loss, logits, retain_graph=True)
    loss.backward()
    params = list(sampler.parameters())
    assert len(params) == 6
    for name, prm in sampler.named_parameters():
        assert prm.grad is not None, "%s got no gradient" % name
        assert torch.isfinite(prm.grad).all() and prm.grad.abs().max().item() > 0, name
    eng = model.engine
    eng.forward(clip.detach(), training=True)
    dx = eng.backward(dlogits.contiguous(), need_dx=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(clip.grad), _bits(dx))
