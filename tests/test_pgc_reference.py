"""The float64 restatement of ProjectionGraphConv (tests/pgc_reference.py) pinned before the GPU tests rely on it: an independent
numpy forward, central finite differences of its hand-written backward pass, and the engine's initialisation of centers / variance
(Keras glorot_uniform for the (1, 64, 1, 32) weights: U(-0.0533, 0.0533))."""
import math

import numpy as np
import pytest
import torch

import pgc_reference as R

B, C, T, V, J = 2, 8, 5, 25, 4


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, C, T, V, generator=g, dtype=torch.float64))
    cen = 0.5 * torch.randn(1, C, 1, J, generator=g, dtype=torch.float64)
    var = 0.5 * torch.randn(1, C, 1, J, generator=g, dtype=torch.float64)
    W = 0.3 * torch.randn(1, C, C, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    return x, cen, var, W, b


def _numpy_forward(x, cen, var, W, b):
    """the reference's call() line by line (models/stpgcn.py:23-47), z materialised"""
    x, cen, var, W, b = (t.numpy() for t in (x, cen, var, W, b))
    N, Cc, Tt, Vv = x.shape
    z = (x.reshape(N, Cc, -1, 1) - cen) / (1 / (1 + np.exp(-var)))           # (N, C, P, J)
    q = np.maximum(np.sum(z ** 2, axis=1), 1e-12) * (-1 / 2)                  # (N, P, J)
    q = np.exp(q - q.max(-1, keepdims=True))
    q /= q.sum(-1, keepdims=True)
    zz = np.sum(q[:, None] * z, axis=-2) / np.sum(q, axis=-2, keepdims=True)  # (N, C, J)
    zz = zz / np.sqrt(np.maximum(np.sum(zz ** 2, axis=-1, keepdims=True), 1e-12))
    A = np.matmul(np.transpose(zz, (0, 2, 1)), zz)
    g = np.einsum("cf,ncv->nfv", W[0], zz) + b[None, :, None]
    g = np.einsum("ncv,nvw->ncw", g, A)
    xp = np.transpose(np.matmul(q, np.transpose(g, (0, 2, 1))), (0, 2, 1)).reshape(N, -1, Tt, Vv)
    return x + xp, q, zz, A


def test_forward_matches_an_independent_numpy_restatement():
    args = _inputs()
    out, ctx = R.pgc_forward(*args)
    ref, q, zn, A = _numpy_forward(*args)
    for got, want in ((out, ref), (ctx["q"], q), (ctx["zn"], zn), (ctx["A"], A)):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_backward_matches_central_finite_differences():
    args = list(_inputs(1))
    g = torch.Generator().manual_seed(2)
    dout = torch.randn(B, C, T, V, generator=g, dtype=torch.float64)
    _, ctx = R.pgc_forward(*args)
    grads = R.pgc_backward(ctx, dout)

    def f(a):
        return (R.pgc_forward(*a)[0] * dout).sum().item()

    h = 1e-6
    rng = np.random.default_rng(3)
    for i, (a, ga) in enumerate(zip(args, grads)):
        flat = a.view(-1)
        idx = rng.choice(flat.numel(), size=min(24, flat.numel()), replace=False)
        for k in idx:
            old = flat[k].item()
            flat[k] = old + h
            fp = f(args)
            flat[k] = old - h
            fm = f(args)
            flat[k] = old
            fd = (fp - fm) / (2 * h)
            an = ga.reshape(-1)[k].item()
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)), (i, int(k), fd, an)


def test_autograd_function_matches_the_plain_backward():
    args = [t.clone().requires_grad_(True) for t in _inputs(4)]
    out = R.PGC.apply(*args)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    out.backward(dout)
    _, ctx = R.pgc_forward(*[t.detach() for t in args])
    for a, want in zip(args, R.pgc_backward(ctx, dout)):
        assert torch.equal(a.grad, want)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_centers_and_variance_init_is_glorot_uniform(seed):
    from sar_amd.stpgcn import glorot_uniform
    limit = math.sqrt(6.0 / (64 + 32 * 64))
    assert abs(limit - 0.0533) < 1e-4
    w = glorot_uniform((1, 64, 1, 32), torch.Generator().manual_seed(seed))
    assert w.shape == (1, 64, 1, 32)
    assert w.abs().max().item() <= limit
    assert abs(w.std().item() - limit / math.sqrt(3)) <= 0.05 * limit / math.sqrt(3)
