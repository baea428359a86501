"""The float64 restatements of tests/gcn_reference.py against cases that can be worked out by hand, against the oracle where the two
overlap, and their analytic gradients against finite differences (torch.autograd.gradcheck)."""
import torch

import gcn_reference as R
from oracle import stgcn as O


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_graph_conv_with_identity_adjacency_is_the_pointwise_convolution():
    x, k, b = _rand(2, 3, 5), _rand(1, 3, 4, seed=1), _rand(4, seed=2)
    A = torch.eye(5, dtype=torch.float64).expand(2, 5, 5)
    want = torch.stack([k[0].t() @ x[n] + b[:, None] for n in range(2)])
    assert torch.allclose(R.graph_conv(x, A, k, b), want, rtol=0, atol=1e-14)


def test_graph_conv_with_a_permutation_per_sample_moves_the_joints():
    """A[n, v, w] = 1 iff w = perm_n(v): out[n, :, perm_n(v)] = conv(x)[n, :, v], a different permutation per sample"""
    x, k, b = _rand(2, 3, 5), _rand(1, 3, 4, seed=1), _rand(4, seed=2)
    perms = [torch.tensor([2, 0, 4, 1, 3]), torch.tensor([1, 2, 3, 4, 0])]
    A = torch.zeros(2, 5, 5, dtype=torch.float64)
    for n, p in enumerate(perms):
        A[n, torch.arange(5), p] = 1.0
    out = R.graph_conv(x, A, k, b)
    conv = R.graph_conv(x, torch.eye(5, dtype=torch.float64).expand(2, 5, 5), k, b)
    for n, p in enumerate(perms):
        assert torch.equal(out[n][:, p], conv[n])


def test_graph_conv_with_a_one_hot_kernel_selects_a_channel():
    x = _rand(2, 3, 5)
    A = _rand(2, 5, 5, seed=3)
    k = torch.zeros(1, 3, 2, dtype=torch.float64)
    k[0, 2, 0], k[0, 0, 1] = 1.0, 1.0                      # filter 0 reads channel 2, filter 1 reads channel 0
    out = R.graph_conv(x, A, k, torch.zeros(2, dtype=torch.float64))
    for n in range(2):
        assert torch.allclose(out[n, 0], x[n, 2] @ A[n], rtol=0, atol=1e-14)
        assert torch.allclose(out[n, 1], x[n, 0] @ A[n], rtol=0, atol=1e-14)


def test_adj_graph_conv_channel_order_is_slice_major():
    """a kernel that is one-hot on output channel k F + m makes filter m the input channel contracted with slice k alone"""
    K, F, C, V = 3, 2, 4, 5
    x, A = _rand(2, C, 3, V), _rand(K, V, V, seed=4)
    for k in range(K):
        kern = torch.zeros(1, 1, C, K * F, dtype=torch.float64)
        kern[0, 0, 1, k * F + 1] = 1.0
        out = R.adj_graph_conv(x, A, kern, torch.zeros(K * F, dtype=torch.float64))
        assert torch.allclose(out[:, 1], x[:, 1] @ A[k], rtol=0, atol=1e-14)
        assert torch.equal(out[:, 0], torch.zeros_like(out[:, 0]))


def test_adj_graph_conv_agrees_with_the_oracle_graph_conv_td():
    x, A, k, b = _rand(2, 4, 3, 5), _rand(3, 5, 5, seed=4), _rand(1, 1, 4, 6, seed=5), _rand(6, seed=6)
    assert torch.allclose(R.adj_graph_conv(x, A, k, b), O.graph_conv_td(x, k, b, A), rtol=0, atol=1e-13)


def test_gradients_against_finite_differences():
    req = lambda t: t.requires_grad_(True)
    assert torch.autograd.gradcheck(R.graph_conv, (req(_rand(2, 3, 4)), req(_rand(2, 4, 4, seed=1)), req(_rand(1, 3, 2, seed=2)),
                                                   req(_rand(2, seed=3))))
    assert torch.autograd.gradcheck(R.adj_graph_conv, (req(_rand(2, 3, 2, 4)), req(_rand(2, 4, 4, seed=1)),
                                                       req(_rand(1, 1, 3, 4, seed=2)), req(_rand(4, seed=3))))
