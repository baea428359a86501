"""CPU: the restatement of GPool / SGCN that the GPU tests are held against (tests/gpool_reference.py) is itself checked -- its
hand-written backward against autograd of its literal forward in float64 and against central differences, `keep` against the
reference's float32 product, the selection's order, and the SGCN restatement against torch.einsum."""
import pytest
import torch

import gpool_reference as R

SHAPES = [(3, 5, 7, 25, 3, 0.5), (2, 64, 12, 25, 3, 0.8), (4, 16, 9, 64, 1, 0.3), (2, 3, 300, 25, 3, 0.5), (3, 8, 6, 25, 2, 1.0),
          (2, 6, 5, 33, 4, 0.7), (1, 2, 1, 2, 1, 0.5)]


def _rel(a, b):
    return ((a - b).abs().max() / max(b.abs().max().item(), 1e-300)).item()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hand_backward_matches_autograd(shape):
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    xs, As, ps = (t.clone().requires_grad_() for t in (x, A, p))
    out, A_out, y, idx = R.forward(xs, As, ps, shape[5])
    ((out * dout).sum() + (A_out * dA_out).sum()).backward()
    dx, dp, dA = R.backward(x, A, p, idx, y.detach(), dout, dA_out)
    assert _rel(dx, xs.grad) < 1e-10 and _rel(dA, As.grad) < 1e-10
    if shape[1] * shape[2] == 1:                       # ph = +-1 whatever p is: dp is zero
        assert dp.abs().max().item() < 1e-10 and ps.grad.abs().max().item() < 1e-10
    else:
        assert _rel(dp, ps.grad) < 1e-10
    only_x = R.backward(x, A, p, idx, y.detach(), dout, None)
    only_A = R.backward(x, A, p, idx, y.detach(), None, dA_out)
    assert only_x[2] is None and only_A[0] is None and only_A[1] is None
    assert torch.equal(only_x[0], dx) and torch.equal(only_A[2], dA)


def test_dp_matches_central_differences():
    shape = (3, 5, 7, 25, 3, 0.5)
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    out, _, y, idx = R.forward(x, A, p, shape[5])
    assert R.min_gap(y) > 1e-4                          # the selection does not change under the perturbation
    _, dp, _ = R.backward(x, A, p, idx, y, dout, dA_out)
    h = 1e-6
    for j in (0, 11, 34):
        e = torch.zeros_like(p)
        e[j] = h
        fp, fm = R.forward(x, A, p + e, shape[5]), R.forward(x, A, p - e, shape[5])
        assert torch.equal(fp[3], idx) and torch.equal(fm[3], idx)
        fd = (((fp[0] - fm[0]) * dout).sum() / (2 * h)).item()
        assert abs(fd - dp[j].item()) < 1e-6 * max(1.0, abs(fd)), (j, fd, dp[j].item())


def test_clamped_norm_branch():
    """p = 0: ph = 0, every score 0, dp = dph * 1e6"""
    shape = (2, 3, 4, 5, 1, 0.6)
    x, A, p, dout, dA_out = R.make_case(shape, 0)
    p = torch.zeros_like(p)
    ps = p.clone().requires_grad_()
    out, _, y, idx = R.forward(x, A, ps, shape[5])
    assert torch.equal(idx, torch.arange(3).expand(2, 3))
    (out * dout).sum().backward()
    _, dp, _ = R.backward(x, A, p, idx, y.detach(), dout, None)
    assert _rel(dp, ps.grad) < 1e-10 and dp.abs().max().item() > 1.0


@pytest.mark.parametrize("V,keeprate,keep", [(25, .5, 12), (25, .8, 20), (25, .7, 17), (25, .28, 7), (64, .3, 19), (33, .7, 23), (2, .5, 1),
                                             (25, 1.0, 25)])
def test_keep(V, keeprate, keep):
    assert R.keep_of(keeprate, V) == keep


def test_keep_of_nothing_raises():
    with pytest.raises(ValueError):
        R.keep_of(.03, 25)
    with pytest.raises(ValueError):
        R.keep_of(0.0, 25)
    with pytest.raises(ValueError):
        R.keep_of(1.5, 25)


def test_selection_order():
    nan = float("nan")
    y = torch.tensor([[1.0, 3.0, 3.0, nan, -1.0, float("-inf")], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [nan, nan, 2.0, nan, 2.0, 5.0]])
    assert R.argsort_desc(y).tolist() == [[1, 2, 0, 4, 5, 3], [0, 1, 2, 3, 4, 5], [5, 2, 4, 0, 1, 3]]


@pytest.mark.parametrize("shape", [(3, 5, 7, 12, 3, 6), (2, 8, 4, 25, 3, 16), (4, 16, 9, 19, 4, 24)], ids=lambda s: "x".join(map(str, s)))
def test_sgcn_restatement_matches_einsum(shape):
    N, C, T, V, K, F = shape
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, C, T, V, generator=g, dtype=torch.float64)
    A = torch.rand(N, K, V, V, generator=g, dtype=torch.float64)
    kernel = torch.randn(1, 1, C, K * F, generator=g, dtype=torch.float64)
    bias = torch.randn(K * F, generator=g, dtype=torch.float64)
    conv = torch.einsum("nctv,cm->nmtv", x, kernel[0, 0]) + bias.view(1, -1, 1, 1)
    want = torch.einsum("nkctv,nkvw->nctw", conv.view(N, K, F, T, V), A)
    assert _rel(R.sgcn_forward(x, A, kernel, bias), want) < 1e-12
