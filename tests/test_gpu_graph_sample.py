"""The per-sample adjacency contraction (csrc/graph_sample.hip; models/gcn.py:22-36 GraphConv's einsum 'ncv,nvw->ncw' and its two
gradients) through sar_amd.ops, against a float64 einsum and its autograd.

Bar: rel_err < 2e-5, the project's per-kernel bar (tests/test_gpu_adjacency.py).  Inputs are seeded standard normal: on the CPU a
plain float32 torch.bmm of the SAME inputs stays at 4.9e-7 (fwd), 7.1e-7 (bwd_data), 5.8e-7 (dadj) of the float64 result at the
largest case (N, F, V) = (2, 256, 512), more than twenty times under the bar, so no other input scale is needed."""
import functools

import pytest
import torch

from sar_amd import _lib
from sar_amd.ops import graph_sample_bwd_data, graph_sample_dA, graph_sample_fwd
from util import rel_err

pytestmark = pytest.mark.gpu
BAR = 2e-5
CASES = [(3, 40, 25), (2, 64, 33), (1, 5, 1), (2, 256, 512)]
POISON = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cn(x):
    """(N, C, V) -> CN matrix [C][N V]"""
    N, Cc, V = x.shape
    return x.permute(1, 0, 2).reshape(Cc, N * V).contiguous()


@functools.lru_cache(maxsize=None)
def case(N, F, V):
    """inputs and the float64 reference of one case, computed once and shared (never modified)"""
    g = torch.Generator().manual_seed(1000 * N + 10 * F + V)
    y, A, dout = torch.randn(N, F, V, generator=g), torch.randn(N, V, V, generator=g), torch.randn(N, F, V, generator=g)
    yd, Ad = y.double().requires_grad_(True), A.double().requires_grad_(True)
    ref = torch.einsum("ncv,nvw->ncw", yd, Ad)
    gy, gA = torch.autograd.grad(ref, (yd, Ad), dout.double())
    return y, A, dout, ref.detach(), gy, gA


def run(dev, y, A, dout, pad=0):
    """the three kernels on CN operands with `pad` poisoned columns behind the N V live ones -> (out, dy, dA)"""
    N, F, V = y.shape
    n = N * V

    def padded(src):
        buf = torch.full((F, n + pad), POISON, device=dev)
        if src is not None:
            buf[:, :n] = cn(src).to(dev)
        return buf
    yc, dc, out, dy = padded(y), padded(dout), padded(None), padded(None)
    Ac = A.to(dev).contiguous()
    dA = torch.full((N, V, V), POISON, device=dev)
    graph_sample_fwd(yc, Ac, out, F, V, N)
    graph_sample_bwd_data(dc, Ac, dy, F, V, N)
    graph_sample_dA(yc, dc, dA, F, V, N)
    torch.cuda.synchronize()
    return out, dy, dA


@pytest.mark.parametrize("N,F,V", CASES)
def test_three_kernels_against_float64(dev, N, F, V):
    y, A, dout, ref, gy, gA = case(N, F, V)
    out, dy, dA = run(dev, y, A, dout)
    errs = rel_err(out, cn(ref)), rel_err(dy, cn(gy)), rel_err(dA, gA)
    print("graph_sample (N, F, V) = (%d, %d, %d): fwd %.2e  bwd_data %.2e  dadj %.2e" % ((N, F, V) + errs))
    assert max(errs) < BAR


def test_padding_columns_are_neither_read_nor_written(dev):
    """ld > N V: the columns behind the live ones hold a poison value, come back untouched and do not reach any result"""
    N, F, V = 3, 40, 25
    y, A, dout, ref, gy, gA = case(N, F, V)
    out, dy, dA = run(dev, y, A, dout, pad=7)
    n = N * V
    assert out.stride(0) == n + 7
    assert bool((out[:, n:] == POISON).all()) and bool((dy[:, n:] == POISON).all())
    errs = rel_err(out[:, :n], cn(ref)), rel_err(dy[:, :n], cn(gy)), rel_err(dA, gA)
    print("graph_sample with ld = N V + 7: fwd %.2e  bwd_data %.2e  dadj %.2e" % errs)
    assert max(errs) < BAR
    tight = run(dev, y, A, dout)
    assert torch.equal(out[:, :n], tight[0]) and torch.equal(dy[:, :n], tight[1]) and torch.equal(dA, tight[2])


@pytest.mark.parametrize("N,F,V", [(3, 40, 25), (3, 70, 130)])
def test_a_sample_does_not_depend_on_the_batch(dev, N, F, V):
    """N = 3 at once, then each sample alone: bitwise equal (the second shape takes the tiled kernel with more than one row block)"""
    g = torch.Generator().manual_seed(77 + V)
    y, A, dout = torch.randn(N, F, V, generator=g), torch.randn(N, V, V, generator=g), torch.randn(N, F, V, generator=g)
    out, dy, dA = run(dev, y, A, dout)
    for i in range(N):
        o1, d1, a1 = run(dev, y[i:i + 1], A[i:i + 1], dout[i:i + 1])
        assert torch.equal(o1, out[:, i * V:(i + 1) * V]) and torch.equal(d1, dy[:, i * V:(i + 1) * V]) and torch.equal(a1[0], dA[i])


@pytest.mark.parametrize("N,F,V", [(3, 40, 25), (2, 256, 512)])
def test_two_launches_are_bitwise_equal(dev, N, F, V):
    y, A, dout = case(N, F, V)[:3]
    first, second = run(dev, y, A, dout), run(dev, y, A, dout)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_rejected_arguments_return_the_error_code_and_launch_nothing(dev):
    lib = _lib.load()
    F, N = 4, 2
    big = torch.full((F, N * 513), POISON, device=dev)         # large enough for every shape tried: nothing below may touch it
    src = torch.zeros((F, N * 513), device=dev)
    A = torch.zeros((N, 513, 513), device=dev)
    p, s, a = big.data_ptr(), src.data_ptr(), A.data_ptr()
    fns = [lambda V, ld, x=s, t=a, o=p: lib.sar_graph_sample_fwd_f32(x, ld, t, o, ld, F, V, N, None),
           lambda V, ld, x=s, t=a, o=p: lib.sar_graph_sample_bwd_data_f32(x, ld, t, o, ld, F, V, N, None),
           lambda V, ld, x=s, t=a, o=p: lib.sar_graph_sample_dadj_f32(x, ld, x, ld, o, F, V, N, None)]
    for fn in fns:
        assert fn(513, N * 513) == _lib.SAR_E_UNSUP            # valid, but beyond what the kernel is built for
        assert fn(0, 64) == _lib.SAR_E_ARG
        assert fn(25, N * 25 - 1) == _lib.SAR_E_ARG            # ld < N V
        assert fn(25, N * 25, x=None) == _lib.SAR_E_ARG        # null pointers
        assert fn(25, N * 25, o=None) == _lib.SAR_E_ARG
    assert lib.sar_graph_sample_fwd_f32(s, 50, None, p, 50, F, 25, N, None) == _lib.SAR_E_ARG
    assert lib.sar_graph_sample_fwd_f32(s, 50, a, p, 50, 0, 25, N, None) == _lib.SAR_E_ARG
    assert lib.sar_graph_sample_fwd_f32(s, 50, a, p, 50, F, 25, 0, None) == _lib.SAR_E_ARG
    torch.cuda.synchronize()
    assert bool((big == POISON).all())
