"""GPU: GPool and SGCN (models/stgcn_debug.py, csrc/gpool.hip, sar_amd.ops.gpool_forward / gpool_backward) against the float64
restatement of tests/gpool_reference.py.

The selection is discrete, so every parity case first asserts a precondition ON THE REFERENCE ALONE: in every sample consecutive
sorted scores differ by at least GAP = 1e-4 max |y| (about 300 times the float32 restatement's distance in y, 1e-7 .. 5e-7).  Then idx
equals the reference exactly and out, A_out, dx, dA, dp pass rel_err < TOL = 1e-4; a summed quantity (y, dx, dp) that misses TOL is
judged against eight times the float32 restatement's own distance from float64, both printed (the rule of tests/test_gpu_stpgcn.py)."""
import functools
import math

import pytest
import torch

import gpool_reference as R
from util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
GAP = 1e-4
SUMS = ("y", "dx", "dp")

# (N, C, T, V, K, keeprate) -> the seed whose float64 scores meet the gap precondition (checked on the CPU)
CASES = {
    (3, 5, 7, 25, 3, 0.5): 0,           # nothing a multiple of anything
    (2, 64, 12, 25, 3, 0.8): 0,
    (4, 16, 9, 64, 1, 0.3): 2,          # V at its limit
    (2, 3, 300, 25, 3, 0.5): 0,         # the workload's run length
    (3, 8, 6, 25, 2, 1.0): 0,           # keep = V: a pure re-ordering
    (2, 6, 5, 33, 4, 0.7): 1,           # V above a half wave
    (1, 2, 1, 2, 1, 0.5): 0,
    (2, 1, 1, 5, 1, 0.6): 9,            # C T = 1: dp is analytically zero
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _judge(name, got, ref64, ref32):
    e = rel_err(got, ref64)
    if e < TOL or name not in SUMS:
        return e
    band = rel_err(ref32, ref64)
    print("%s: kernels %.3e, float32 restatement %.3e from float64" % (name, e, band))
    return 0.0 if e <= 8 * band else e


@functools.lru_cache(maxsize=None)
def _reference(shape, seed, zero_p=False):
    """the case, its float64 results and the float32 restatement's; computed once, never modified"""
    case = R.make_case(shape, seed)
    if zero_p:
        case = case[:2] + (torch.zeros_like(case[2]),) + case[3:]
    x, A, p, dout, dA_out = case
    out, A_out, y, idx = R.forward(x, A, p, shape[5])
    dx, dp, dA = R.backward(x, A, p, idx, y, dout, dA_out)
    c32 = tuple(t.float() for t in case)
    out32, A_out32, y32, idx32 = R.forward(c32[0], c32[1], c32[2], shape[5])
    dx32, dp32, dA32 = R.backward(c32[0], c32[1], c32[2], idx, y32, c32[3], c32[4])
    ref64 = dict(out=out, A_out=A_out, y=y, dx=dx, dp=dp, dA=dA)
    ref32 = dict(out=out32, A_out=A_out32, y=y32, dx=dx32, dp=dp32, dA=dA32)
    return case, idx, idx32, ref64, ref32


def _run(dev, case, keeprate):
    from sar_amd import ops
    x, A, p, dout, dA_out = (t.float().to(dev).contiguous() for t in case)
    out, A_out, saved = ops.gpool_forward(x, A, p, keeprate)
    dx, dp, dA = ops.gpool_backward(x, A, saved, dout, dA_out)
    torch.cuda.synchronize()
    return dict(out=out, A_out=A_out, y=saved[2], dx=dx, dp=dp.view(-1, 1), dA=dA, idx=saved[0], s=saved[3], pos=saved[1])


@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_parity_against_float64(dev, shape):
    case, idx, idx32, ref64, ref32 = _reference(shape, CASES[shape])
    gap = R.min_gap(ref64["y"])
    assert gap >= GAP, "precondition on the reference: the smallest score gap is %.2e of max |y| (seed %d)" % (gap, CASES[shape])
    assert torch.equal(idx32, idx), "the float32 restatement selects other vertices"
    got = _run(dev, case, shape[5])
    assert torch.equal(got["idx"].cpu().long(), idx)
    N, C, T, V = shape[:4]
    pos = torch.full((N, V), -1, dtype=torch.long).scatter(1, idx, torch.arange(idx.shape[1]).expand(N, -1))
    assert torch.equal(got["pos"].cpu().long(), pos)
    worst = {}
    for k in ("y", "out", "A_out", "dx", "dA", "dp"):
        if k == "dp" and C * T == 1:                  # ph = +-1: dp = (dph - ph <dph, ph>) / |p| = 0; what is left is rounding of dph / |p|
            x, _, p, dout, _ = case
            sel = idx[:, None, :]
            s = torch.sigmoid(ref64["y"].gather(1, idx))
            dph = ((dout.reshape(N, 1, -1) * x.reshape(N, 1, V).gather(2, sel)).sum(1) * s * (1 - s) * x.reshape(N, V).gather(1, idx)).sum()
            size = got["dp"].abs().max().item()
            print("dp (C T = 1): %.3e absolute, |dph| / |p| = %.3e" % (size, abs(dph.item()) / p.norm().item()))
            worst[k] = size / max(abs(dph.item()) / p.norm().item(), 1e-30)
            continue
        worst[k] = _judge(k, got[k], ref64[k], ref32[k])
    print(shape, {k: "%.2e" % v for k, v in worst.items()})
    assert all(v < TOL for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ ties and degenerate scores
def test_equal_joints_come_out_in_ascending_index(dev):
    shape = (3, 5, 7, 25, 3, 1.0)
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    x[..., 17] = x[..., 3]
    x[..., 9] = x[..., 3]
    got = _run(dev, (x, A, p, dout, dA_out), 1.0)
    y, pos = got["y"].cpu(), got["pos"].cpu()
    assert torch.equal(y[:, 3], y[:, 17]) and torch.equal(y[:, 3], y[:, 9])
    assert torch.equal(pos[:, 9], pos[:, 3] + 1) and torch.equal(pos[:, 17], pos[:, 3] + 2)
    assert torch.equal(got["idx"].cpu().long(), R.argsort_desc(y))


def test_empty_sample_keeps_the_first_vertices(dev):
    shape = (3, 5, 7, 25, 3, 0.5)
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    x[2] = 0                                           # the empty second body of a clip
    got = _run(dev, (x, A, p, dout, dA_out), 0.5)
    assert torch.equal(got["idx"][2].cpu(), torch.arange(12, dtype=torch.int32))
    assert torch.equal(got["s"][2].cpu(), torch.full((12,), 0.5))
    assert bool((got["out"][2] == 0).all())
    for k in ("out", "A_out", "dx", "dA", "dp"):
        assert bool(torch.isfinite(got[k]).all()), k


def test_zero_projection_vector_takes_the_clamped_branch(dev):
    shape = (3, 5, 7, 25, 3, 0.5)
    case, idx, _, ref64, _ = _reference(shape, 0, True)
    got = _run(dev, case, 0.5)
    assert torch.equal(got["idx"].cpu().long(), idx) and torch.equal(idx, torch.arange(12).expand(3, 12))
    assert ref64["dp"].abs().max().item() > 1e3        # dph * 1e6
    for k in ("out", "dx", "dp"):
        assert rel_err(got[k], ref64[k]) < TOL, k


def test_nan_joint_is_never_selected(dev):
    shape = (3, 5, 7, 25, 3, 0.5)
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    x[0, :, :, 5] = float("nan")
    x[0, 2, 3, 20] = float("nan")
    x[1] = float("nan")                                # every score NaN
    got = _run(dev, (x, A, p, dout, dA_out), 0.5)
    idx = got["idx"].cpu().long()
    assert 5 not in idx[0].tolist() and 20 not in idx[0].tolist()
    assert torch.equal(idx[1], torch.arange(12))
    for n in range(3):
        assert len(set(idx[n].tolist())) == 12 and 0 <= int(idx[n].min()) and int(idx[n].max()) < 25
    assert torch.equal(idx, R.argsort_desc(got["y"].cpu())[:, :12])
    assert bool(torch.isfinite(got["out"][0]).all()) and bool(torch.isfinite(got["out"][2]).all())
    assert bool((got["dx"][0, :, :, 5] == 0).all())    # no gradient reaches a joint that was not selected and has no score share


# ------------------------------------------------------------------------------------------------ determinism and independence
def test_two_runs_are_bitwise_equal(dev):
    shape = (2, 64, 12, 25, 3, 0.8)
    case = _reference(shape, CASES[shape])[0]
    a, b = _run(dev, case, shape[5]), _run(dev, case, shape[5])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_sample_does_not_depend_on_the_batch(dev):
    """the benchmark shape, generated on the GPU: every 8-sample slice is bitwise the N = 8 run on that slice"""
    from sar_amd import ops
    N, C, T, V, K, keeprate = 128, 64, 300, 25, 3, 0.5
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.relu(torch.randn(N, C, T, V, generator=g, device=dev))
    A = torch.rand(N, K, V, V, generator=g, device=dev) * (torch.rand(N, K, V, V, generator=g, device=dev) < 0.3)
    p = (torch.rand(C * T, 1, generator=g, device=dev) * 2 - 1) * math.sqrt(6.0 / (C * T + 1))
    dout = torch.randn(N, C, T, 12, generator=g, device=dev)
    dA_out = torch.randn(N, K, 12, 12, generator=g, device=dev)
    out, A_out, saved = ops.gpool_forward(x, A, p, keeprate)
    dx, _, dA = ops.gpool_backward(x, A, saved, dout, dA_out)
    for n0 in range(0, N, 8):
        sl = slice(n0, n0 + 8)
        o8, A8, saved8 = ops.gpool_forward(x[sl], A[sl], p, keeprate)
        dx8, _, dA8 = ops.gpool_backward(x[sl], A[sl], saved8, dout[sl], dA_out[sl])
        for what, whole, part in (("out", out, o8), ("A_out", A_out, A8), ("idx", saved[0], saved8[0]), ("dx", dx, dx8), ("dA", dA, dA8)):
            assert torch.equal(whole[sl], part), "%s of samples %d..%d depends on the batch" % (what, n0, n0 + 7)


def test_cn_views_give_the_nchw_bits(dev):
    """the same case as NCHW tensors and as views of CN matrices [C][ld] (ld > N T V): the CN results are the NCHW bits, permuted"""
    from sar_amd import ops
    shape = (3, 5, 7, 25, 3, 0.5)
    case = _reference(shape, CASES[shape])[0]
    N, C, T, V = shape[:4]
    x, A, p, dout, dA_out = (t.float().to(dev).contiguous() for t in case)
    keep = dout.shape[3]
    out, A_out, saved = ops.gpool_forward(x, A, p, shape[5])
    dx, dp, dA = ops.gpool_backward(x, A, saved, dout, dA_out)

    def cn(t, W, pad=3):
        m = torch.full((C, N * T * W + pad), float("nan"), dtype=torch.float32, device=dev)
        view = m[:, :N * T * W].view(C, N, T, W).permute(1, 0, 2, 3)
        if t is not None:
            view.copy_(t)
        return view
    xc, oc, dc, gc = cn(x, V), cn(None, keep), cn(dout, keep), cn(None, V)
    assert xc.stride() == (T * V, N * T * V + 3, V, 1)
    out_c, A_out_c, saved_c = ops.gpool_forward(xc, A, p, shape[5], out=oc)
    dx_c, dp_c, dA_c = ops.gpool_backward(xc, A, saved_c, dc, dA_out, dx=gc)
    assert out_c.data_ptr() == oc.data_ptr() and dx_c.data_ptr() == gc.data_ptr()
    for what, a, b in (("out", out, out_c), ("A_out", A_out, A_out_c), ("idx", saved[0], saved_c[0]), ("y", saved[2], saved_c[2]),
                       ("dx", dx, dx_c), ("dp", dp, dp_c), ("dA", dA, dA_c)):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------ the module
def _module_case(dev, shape=(3, 5, 7, 25, 3, 0.5)):
    case = _reference(shape, CASES[shape])[0]
    return tuple(t.float().to(dev).contiguous() for t in case)


def test_module_builds_lazily_and_trains(dev):
    from models.stgcn_debug import GPool
    x, A, p, dout, dA_out = _module_case(dev)
    layer = GPool(0.5)
    assert layer.projection_vector is None
    out, A_out = layer(x, A, training=True)
    pv = layer.projection_vector
    assert tuple(pv.shape) == (35, 1) and pv.is_cuda and pv.abs().max().item() <= math.sqrt(6.0 / 36)
    assert tuple(out.shape) == (3, 5, 7, 12) and tuple(A_out.shape) == (3, 3, 12, 12)
    opt = torch.optim.SGD(layer.parameters(), lr=0.1)
    before = pv.detach().clone()
    ((out * dout).sum() + (A_out * dA_out).sum()).backward()
    opt.step()
    assert pv.grad is not None and bool(torch.isfinite(pv.grad).all()) and not torch.equal(pv.detach(), before)


def test_module_state_dict_round_trip_before_the_first_call(dev):
    from models.stgcn_debug import GPool
    x, A, p, dout, dA_out = _module_case(dev)
    src = GPool(0.5)
    src.load_state_dict({"projection_vector": p})
    dst = GPool(0.5)
    dst.load_state_dict(src.state_dict())
    assert torch.equal(dst.projection_vector.detach(), p)
    case, idx, _, ref64, _ = _reference((3, 5, 7, 25, 3, 0.5), 0)
    out, A_out = dst(x, A)
    assert rel_err(out, ref64["out"]) < TOL and rel_err(A_out, ref64["A_out"]) < TOL


def test_module_gradient_of_one_output_alone(dev):
    from models.stgcn_debug import GPool
    x, A, p, dout, dA_out = _module_case(dev)
    case, idx, _, ref64, _ = _reference((3, 5, 7, 25, 3, 0.5), 0)
    layer = GPool(0.5)
    layer.load_state_dict({"projection_vector": p})
    xs, As = x.clone().requires_grad_(), A.clone().requires_grad_()
    out, A_out = layer(xs, As, training=True)
    (out * dout).sum().backward()
    assert As.grad is None and rel_err(xs.grad, ref64["dx"]) < TOL and rel_err(layer.projection_vector.grad, ref64["dp"]) < TOL
    xs, As = x.clone().requires_grad_(), A.clone().requires_grad_()
    layer.zero_grad(set_to_none=True)
    out, A_out = layer(xs, As, training=True)
    (A_out * dA_out).sum().backward()
    assert xs.grad is None and layer.projection_vector.grad is None and rel_err(As.grad, ref64["dA"]) < TOL


def test_module_rejects_what_it_is_not_built_for(dev):
    from models.stgcn_debug import GPool
    x, A, p, dout, dA_out = _module_case(dev)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match=r"\(N, K, V, V\)"):
        GPool(0.5)(x, A[:, 0])
    with pytest.raises(ValueError, match="V <= 64"):
        GPool(0.5)(z(2, 3, 4, 65), z(2, 1, 65, 65))
    with pytest.raises(ValueError):
        GPool(0.0)
    with pytest.raises(ValueError, match="keep"):
        GPool(0.03)(x, A)
    with pytest.raises(ValueError):
        GPool(0.5)(x.cpu(), A.cpu())
    layer = GPool(0.5)
    layer(x, A)
    with pytest.raises(ValueError, match="built for"):
        layer(x[:, :, :6].contiguous(), A)


# ------------------------------------------------------------------------------------------------ SGCN
def _sgcn_case(shape, seed=0):
    N, C, T, V, K, F = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, T, V, generator=g, dtype=torch.float64)
    A = torch.rand(N, K, V, V, generator=g, dtype=torch.float64) * (torch.rand(N, K, V, V, generator=g) < 0.3)
    kernel = torch.randn(1, 1, C, K * F, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (K * F))
    bias = torch.randn(K * F, generator=g, dtype=torch.float64)
    dout = torch.randn(N, F, T, V, generator=g, dtype=torch.float64)
    return x, A, kernel, bias, dout


@pytest.mark.parametrize("shape", [(3, 5, 7, 12, 3, 6), (2, 64, 12, 25, 3, 64), (4, 16, 9, 19, 4, 24)], ids=lambda s: "x".join(map(str, s)))
def test_sgcn_parity_against_float64(dev, shape):
    from models.stgcn_debug import SGCN
    N, C, T, V, K, F = shape
    case = _sgcn_case(shape)
    leaves = [t.clone().requires_grad_() for t in case[:4]]
    want = R.sgcn_forward(*leaves)
    (want * case[4]).sum().backward()
    layer = SGCN(F, kernel_size=K)
    layer.load_state_dict({"kernel": case[2].float().to(dev), "bias": case[3].float().to(dev)})
    xs, As = (t.float().to(dev).requires_grad_() for t in case[:2])
    out, A_same = layer(xs, As, training=True)
    assert A_same is As and tuple(out.shape) == (N, F, T, V)
    (out * case[4].float().to(dev)).sum().backward()
    errs = {"out": rel_err(out, want), "dx": rel_err(xs.grad, leaves[0].grad), "dA": rel_err(As.grad, leaves[1].grad),
            "dkernel": rel_err(layer.kernel.grad, leaves[2].grad), "dbias": rel_err(layer.bias.grad, leaves[3].grad)}
    print(shape, {k: "%.2e" % v for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs


def test_sgcn_rejects_what_it_is_not_built_for(dev):
    from models.stgcn_debug import SGCN
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    for K, V in ((5, 12), (3, 33), (7, 11), (4, 20)):           # K = 5, V = 33, K V = 77, K V = 80
        with pytest.raises(ValueError, match="K <= 4, V <= 32 and K \\* V <= 76"):
            SGCN(4, kernel_size=K)(z(2, 3, 4, V), z(2, K, V, V))
    with pytest.raises(ValueError):
        SGCN(4)(z(2, 3, 4, 12), z(3, 12, 12))
    with pytest.raises(ValueError):
        SGCN(4)(z(2, 3, 4, 12).cpu(), z(2, 3, 12, 12).cpu())


# ------------------------------------------------------------------------------------------------ the chain
CHAIN_SEED = 2


def _chain_reference(dtype):
    N, C, T, V, K = 2, 8, 6, 25, 3
    x, A, p1, _, _ = R.make_case((N, C, T, V, K, 0.5), CHAIN_SEED)
    g = torch.Generator().manual_seed(100 + CHAIN_SEED)
    k1 = torch.randn(1, 1, C, K * 32, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (K * 32))
    b1 = torch.randn(K * 32, generator=g, dtype=torch.float64) * 0.1
    p2 = (torch.rand(32 * T, 1, generator=g, dtype=torch.float64) * 2 - 1) * math.sqrt(6.0 / (32 * T + 1))
    k2 = torch.randn(1, 1, 32, K * 16, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (K * 16))
    b2 = torch.randn(K * 16, generator=g, dtype=torch.float64) * 0.1
    names = ("x", "A", "p1", "k1", "b1", "p2", "k2", "b2")
    leaves = {k: t.to(dtype).clone().requires_grad_() for k, t in zip(names, (x, A, p1, k1, b1, p2, k2, b2))}
    h, A1, y1, idx1 = R.forward(leaves["x"], leaves["A"], leaves["p1"], 0.5)
    h = R.sgcn_forward(h, A1, leaves["k1"], leaves["b1"])
    h, A2, y2, idx2 = R.forward(h, A1, leaves["p2"], 0.5)
    h = R.sgcn_forward(h, A2, leaves["k2"], leaves["b2"])
    h.mean(dim=(2, 3)).sum().backward()
    return leaves, (y1.detach(), y2.detach()), (idx1, idx2)


def test_chain_of_pools_and_convolutions(dev):
    """GPool(0.5) -> SGCN(32) -> GPool(0.5) -> SGCN(16) -> mean -> sum under autograd: every leaf gradient against float64"""
    from models.stgcn_debug import GPool, SGCN
    ref, ys, idxs = _chain_reference(torch.float64)
    ref32, _, idxs32 = _chain_reference(torch.float32)
    for y in ys:
        assert R.min_gap(y) >= GAP, "precondition on the reference: score gap %.2e of max |y| (seed %d)" % (R.min_gap(y), CHAIN_SEED)
    assert all(torch.equal(a, b) for a, b in zip(idxs, idxs32)), "the float32 restatement selects other vertices"
    f = lambda k: ref[k].detach().float().to(dev)
    pool1, conv1, pool2, conv2 = GPool(0.5), SGCN(32), GPool(0.5), SGCN(16)
    pool1.load_state_dict({"projection_vector": f("p1")})
    pool2.load_state_dict({"projection_vector": f("p2")})
    conv1.load_state_dict({"kernel": f("k1"), "bias": f("b1")})
    conv2.load_state_dict({"kernel": f("k2"), "bias": f("b2")})
    xs, As = f("x").requires_grad_(), f("A").requires_grad_()
    h, A1 = pool1(xs, As, training=True)
    h, A1 = conv1(h, A1, training=True)
    h, A2 = pool2(h, A1, training=True)
    h, A2 = conv2(h, A2, training=True)
    assert tuple(h.shape) == (2, 16, 6, 6) and tuple(A2.shape) == (2, 3, 6, 6)
    h.mean(dim=(2, 3)).sum().backward()
    got = {"x": xs.grad, "A": As.grad, "p1": pool1.projection_vector.grad, "k1": conv1.kernel.grad, "b1": conv1.bias.grad,
           "p2": pool2.projection_vector.grad, "k2": conv2.kernel.grad, "b2": conv2.bias.grad}
    worst = {}
    for k, gk in got.items():
        e, band = rel_err(gk, ref[k].grad), rel_err(ref32[k].grad, ref[k].grad)
        print("d%s: kernels %.3e, float32 restatement %.3e from float64" % (k, e, band))
        worst[k] = e if not (e < TOL or e <= 8 * band) else 0.0
    assert not any(worst.values()), worst
