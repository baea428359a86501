"""The graph isomorphism aggregation with a per-sample adjacency (csrc/graph_sample.hip, SELF instantiation; models/gcn.py:89-93
GraphIsoConv.call: einsum('ncv,nvw->ncw', x, A + diag(1 + epsilon))) and its gradients through sar_amd.ops, against a float64
einsum and its autograd.

Bars.  fwd, bwd_data, dA: rel_err < 2e-5, the project's per-kernel bar (tests/test_gpu_graph_sample.py); plain float32 torch on the
same inputs stays at or below 5.3e-7 of the float64 result in every case here.  d epsilon = <x, dout> is a sum of products of both
signs, so the float64 scalar can sit near zero and a relative bar on it would be ill-conditioned: the bar is
|got - ref| <= 2e-5 sum|x dout| (float32 torch: at most 4.4e-8 of that scale)."""
import functools

import pytest
import torch

from sar_amd import _lib
from sar_amd.ops import (gin_eps_grad_bn, gin_sample_bwd_data, gin_sample_eps_grad, gin_sample_fwd, graph_sample_bwd_data,
                         graph_sample_dA, graph_sample_fwd)
from util import NAN, SENTINEL, assert_guards_untouched, guarded, rel_err

pytestmark = pytest.mark.gpu
BAR = 2e-5
CASES = [(3, 40, 25), (2, 64, 33), (1, 5, 1), (2, 256, 512)]      # one per tile shape, and the multi-chunk one
EPS = 0.3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cn(x):
    """(N, C, V) -> CN matrix [C][N V]"""
    N, Cc, V = x.shape
    return x.permute(1, 0, 2).reshape(Cc, N * V).contiguous()


@functools.lru_cache(maxsize=None)
def case(N, F, V, binary=False):
    """inputs and the float64 reference of one case, computed once and shared (never modified)"""
    g = torch.Generator().manual_seed(2000 * N + 10 * F + V + (7 if binary else 0))
    x, A, dout = torch.randn(N, F, V, generator=g), torch.randn(N, V, V, generator=g), torch.randn(N, F, V, generator=g)
    if binary:                  # what the reference's comment asks of A: binary, no self connections
        A = (A > 0.5).float() * (1 - torch.eye(V))
    xd, Ad = x.double().requires_grad_(True), A.double().requires_grad_(True)
    ed = torch.tensor(EPS, dtype=torch.float64, requires_grad=True)
    ref = torch.einsum("ncv,nvw->ncw", xd, Ad + torch.diag(torch.ones(V, dtype=torch.float64) + ed))
    gx, gA, ge = torch.autograd.grad(ref, (xd, Ad, ed), dout.double())
    scale = (x.double() * dout.double()).abs().sum().item()
    return x, A, dout, ref.detach(), gx, gA, ge.item(), scale


def run(dev, x, A, dout, eps=EPS, pad=0, keep=None):
    """the four kernels on CN operands with `pad` guard columns -> (out, dx, dA, deps); inputs padded with NaN, outputs with the
    sentinel; keep: receives the whole allocations for the guard checks"""
    N, F, V = x.shape
    n = N * V
    xc, xw = guarded(cn(x).to(dev), pad, NAN, dev)
    dc, dw = guarded(cn(dout).to(dev), pad, NAN, dev)
    out, ow = guarded((F, n), pad, SENTINEL, dev)
    dx, dxw = guarded((F, n), pad, SENTINEL, dev)
    Ac = A.to(dev).contiguous()
    e = torch.tensor(eps, dtype=torch.float32, device=dev)
    dA = torch.full((N, V, V), SENTINEL, device=dev)
    deps = torch.full((), SENTINEL, device=dev)
    gin_sample_fwd(xc, Ac, e, out, F, V, N)
    gin_sample_bwd_data(dc, Ac, e, dx, F, V, N)
    graph_sample_dA(xc, dc, dA, F, V, N)
    gin_sample_eps_grad(xc, dc, deps, F, V, N)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(xw=xw, dw=dw, ow=ow, dxw=dxw, x=cn(x), d=cn(dout))
    return out, dx, dA, deps


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("N,F,V", CASES)
def test_four_kernels_against_float64(dev, N, F, V, binary):
    x, A, dout, ref, gx, gA, ge, scale = case(N, F, V, binary)
    out, dx, dA, deps = run(dev, x, A, dout)
    errs = rel_err(out, cn(ref)), rel_err(dx, cn(gx)), rel_err(dA, gA)
    e_err = abs(deps.item() - ge) / scale
    print("gin_sample (N, F, V) = (%d, %d, %d)%s: fwd %.2e  bwd_data %.2e  dadj %.2e  deps %.2e of sum|x dout|"
          % ((N, F, V, " binary A" if binary else "") + errs + (e_err,)))
    assert max(errs) < BAR
    assert e_err <= BAR


@pytest.mark.parametrize("N,F,V", CASES)
def test_eps_minus_one_is_the_plain_contraction(dev, N, F, V):
    """1 + eps = 0: the self term vanishes and the two kernels equal sar_graph_sample_fwd / bwd_data_f32"""
    x, A, dout = case(N, F, V)[:3]
    out, dx, _, _ = run(dev, x, A, dout, eps=-1.0)
    xc, dc, Ac = cn(x).to(dev), cn(dout).to(dev), A.to(dev).contiguous()
    o0, d0 = torch.empty_like(xc), torch.empty_like(dc)
    graph_sample_fwd(xc, Ac, o0, F, V, N)
    graph_sample_bwd_data(dc, Ac, d0, F, V, N)
    assert torch.equal(out, o0) and torch.equal(dx, d0)


@pytest.mark.parametrize("N,F,V", [(3, 40, 25), (2, 64, 33), (2, 40, 130)])
def test_padding_columns_are_neither_read_nor_written(dev, N, F, V):
    """ld = N V + 7: input padding holds NaN, output padding the sentinel; guards untouched, inputs unchanged, results within the bar
    and the live part bitwise equal to the tight run"""
    g = torch.Generator().manual_seed(5 + V)
    x, A, dout = torch.randn(N, F, V, generator=g), torch.randn(N, V, V, generator=g), torch.randn(N, F, V, generator=g)
    n, k = N * V, {}
    out, dx, dA, deps = run(dev, x, A, dout, pad=7, keep=k)
    assert out.stride(0) == n + 7 and dx.stride(0) == n + 7
    for name in ("xw", "dw"):
        assert_guards_untouched(k[name], (F, n), NAN, what=name)
    for name in ("ow", "dxw"):
        assert_guards_untouched(k[name], (F, n), SENTINEL, what=name)
    assert torch.equal(k["xw"][4:4 + F, :n].cpu(), k["x"]) and torch.equal(k["dw"][4:4 + F, :n].cpu(), k["d"])
    tight = run(dev, x, A, dout)
    assert torch.equal(out, tight[0]) and torch.equal(dx, tight[1]) and torch.equal(dA, tight[2])
    ref = (x.double() * dout.double()).sum().item()
    scale = (x.double() * dout.double()).abs().sum().item()
    assert abs(deps.item() - ref) <= BAR * scale and abs(tight[3].item() - ref) <= BAR * scale
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dx).any())


@pytest.mark.parametrize("N,F,V", [(3, 40, 25), (3, 70, 130)])
def test_a_sample_does_not_depend_on_the_batch(dev, N, F, V):
    """N = 3 at once, then each sample alone: bitwise equal (the second shape takes the tiled kernel with more than one row block)"""
    g = torch.Generator().manual_seed(77 + V)
    x, A, dout = torch.randn(N, F, V, generator=g), torch.randn(N, V, V, generator=g), torch.randn(N, F, V, generator=g)
    out, dx, dA, _ = run(dev, x, A, dout)
    for i in range(N):
        o1, d1, a1, _ = run(dev, x[i:i + 1], A[i:i + 1], dout[i:i + 1])
        assert torch.equal(o1, out[:, i * V:(i + 1) * V]) and torch.equal(d1, dx[:, i * V:(i + 1) * V]) and torch.equal(a1[0], dA[i])


@pytest.mark.parametrize("N,F,V", [(3, 40, 25), (2, 256, 512)])
def test_two_launches_are_bitwise_equal(dev, N, F, V):
    """the eps-gradient reduction included: partials are added in a fixed order, no atomics"""
    x, A, dout = case(N, F, V)[:3]
    first, second = run(dev, x, A, dout), run(dev, x, A, dout)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_eps_grad_vector_and_scalar_paths_agree_with_float64(dev):
    """16-byte rows with a column count that is no multiple of 4 (the vector path's partial last group), and more rows x chunks than
    one workgroup's item (F = 3, N V = 2 * 4100 > 4096 columns per item) on both paths"""
    for N, F, V, pad in ((2, 3, 250, 0), (1, 3, 502, 2), (1, 7, 502, 1), (20, 3, 410, 0), (20, 3, 410, 3)):
        g = torch.Generator().manual_seed(N + F + V)
        x, dout = torch.randn(N, F, V, generator=g), torch.randn(N, F, V, generator=g)
        n = N * V
        xc, _ = guarded(cn(x).to(dev), pad, NAN, dev)
        dc, _ = guarded(cn(dout).to(dev), pad, NAN, dev)
        deps = torch.full((), SENTINEL, device=dev)
        gin_sample_eps_grad(xc, dc, deps, F, V, N)
        ref = (x.double() * dout.double()).sum().item()
        scale = (x.double() * dout.double()).abs().sum().item()
        assert xc.stride(0) == n + pad and abs(deps.item() - ref) <= BAR * scale, (N, F, V, pad, deps.item(), ref)


@pytest.mark.parametrize("C", [1, 12, 700])
def test_eps_grad_from_the_batchnorm_backward(dev, C):
    """sar_gin_eps_grad_bn_f32: bn_eps / (1 + eps) sum_c gamma dgamma rstd^2 against float64 (an fp64 sum of products of fp32 values:
    1e-6 of sum|terms| leaves room for the final rounding only); 1 + eps == 0 leaves deps as it is"""
    g = torch.Generator().manual_seed(C)
    gamma, dgamma, rstd = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    terms = gamma.double() * dgamma.double() * rstd.double() ** 2 * 1e-3 / (1.0 + EPS)
    deps = torch.full((), SENTINEL, device=dev)
    args = gamma.to(dev), dgamma.to(dev), rstd.to(dev), 1e-3
    gin_eps_grad_bn(*args, torch.tensor(EPS, device=dev), deps)
    assert abs(deps.item() - terms.sum().item()) <= 1e-6 * terms.abs().sum().item()
    again = torch.full((), SENTINEL, device=dev)
    gin_eps_grad_bn(*args, torch.tensor(EPS, device=dev), again)
    assert torch.equal(again, deps)
    gin_eps_grad_bn(*args, torch.tensor(-1.0, device=dev), again.fill_(SENTINEL))
    assert again.item() == SENTINEL
    lib, p = _lib.load(), args[0].data_ptr()
    e = torch.zeros((), device=dev)
    for bad in ((None, p, p, C, 1e-3, e.data_ptr(), again.data_ptr()), (p, None, p, C, 1e-3, e.data_ptr(), again.data_ptr()),
                (p, p, None, C, 1e-3, e.data_ptr(), again.data_ptr()), (p, p, p, 0, 1e-3, e.data_ptr(), again.data_ptr()),
                (p, p, p, C, 0.0, e.data_ptr(), again.data_ptr()), (p, p, p, C, 1e-3, None, again.data_ptr()),
                (p, p, p, C, 1e-3, e.data_ptr(), None)):
        assert lib.sar_gin_eps_grad_bn_f32(*bad, None) == _lib.SAR_E_ARG
    torch.cuda.synchronize()
    assert again.item() == SENTINEL


def test_rejected_arguments_return_the_error_code_and_launch_nothing(dev):
    lib = _lib.load()
    F, N = 4, 2
    big = torch.full((F, N * 513), SENTINEL, device=dev)         # large enough for every shape tried: nothing below may touch it
    src = torch.zeros((F, N * 513), device=dev)
    A = torch.zeros((N, 513, 513), device=dev)
    e = torch.zeros((), device=dev)
    p, s, a, ep = big.data_ptr(), src.data_ptr(), A.data_ptr(), e.data_ptr()
    fns = [lambda V, ld, x=s, t=a, q=ep, o=p: lib.sar_gin_sample_fwd_f32(x, ld, t, q, o, ld, F, V, N, None),
           lambda V, ld, x=s, t=a, q=ep, o=p: lib.sar_gin_sample_bwd_data_f32(x, ld, t, q, o, ld, F, V, N, None)]
    for fn in fns:
        assert fn(513, N * 513) == _lib.SAR_E_UNSUP            # valid, but beyond what the kernel is built for
        assert fn(0, 64) == _lib.SAR_E_ARG
        assert fn(25, N * 25 - 1) == _lib.SAR_E_ARG            # ld < N V
        assert fn(25, N * 25, x=None) == _lib.SAR_E_ARG        # null x / A / eps / out
        assert fn(25, N * 25, t=None) == _lib.SAR_E_ARG
        assert fn(25, N * 25, q=None) == _lib.SAR_E_ARG
        assert fn(25, N * 25, o=None) == _lib.SAR_E_ARG
    eg = lambda V, ld, x=s, d=s, sc=p, o=p + 4096: lib.sar_gin_sample_eps_grad_f32(x, ld, d, ld, F, V, N, sc, o, None)
    assert eg(513, N * 513) == _lib.SAR_E_UNSUP
    assert eg(0, 64) == _lib.SAR_E_ARG
    assert eg(25, N * 25 - 1) == _lib.SAR_E_ARG
    assert eg(25, N * 25, x=None) == _lib.SAR_E_ARG
    assert eg(25, N * 25, d=None) == _lib.SAR_E_ARG
    assert eg(25, N * 25, sc=None) == _lib.SAR_E_ARG           # null scratch / deps
    assert eg(25, N * 25, o=None) == _lib.SAR_E_ARG
    assert lib.sar_gin_sample_eps_grad_scratch_floats(0, 25, N) == _lib.SAR_E_ARG
    assert lib.sar_gin_sample_eps_grad_scratch_floats(F, 25, N) == F
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all())
