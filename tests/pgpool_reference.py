"""Restatement of ProjectionGraphPool (the reference's models/stpgcnp.py:11-38) with a hand-written backward pass, for the tests of
csrc/pgpool.hip and models/stpgcnp.py.  It runs in the dtype of its inputs: float64 is the oracle, float32 (the same code, the
distance in difference form) gives the band a float32 implementation can be held to.

pool_forward / pool_backward: the per-column distances are formed one vertex at a time, so z = (x - centers) / s -- (N, C, P, J)
in the literal formulation -- is never held for all vertices at once (pinned against the literal formulation under torch
autograd and against central finite differences in tests/test_pgpool_reference.py).  Pool wraps the pair as an autograd function.
A vertex with qs == 0 gives 0 / 0, as in the reference."""
import math

import torch

EPS = 1e-12


def pool_forward(x, centers, variance):
    """x (B, C, ...) ; centers / variance (1, C, 1, J).  Returns (zn (B, C, J), A_out (B, J, J), ctx)."""
    B, C = x.shape[0], x.shape[1]
    x = x.reshape(B, C, -1)
    cen, s = centers.reshape(C, -1), torch.sigmoid(variance.reshape(C, -1))
    J = cen.shape[1]
    d = torch.stack([(((x - cen[:, j, None]) / s[:, j, None]) ** 2).sum(1) for j in range(J)], -1)     # (B, P, J)
    q = torch.softmax(torch.clamp(d, min=EPS) * -0.5, -1)
    S = torch.einsum("bcp,bpj->bcj", x, q)
    qs = q.sum(1)[:, None, :]
    zp = (S - cen * qs) / (s * qs)
    n2 = (zp * zp).sum(-1)
    n = torch.sqrt(torch.clamp(n2, min=EPS))
    zn = zp / n[..., None]
    A = torch.einsum("bci,bcj->bij", zn, zn)
    return zn, A, dict(x=x, cen=cen, s=s, d=d, q=q, S=S, qs=qs, zp=zp, n2=n2, n=n, zn=zn)


def pool_backward(ctx, dz, dA):
    """-> (dx (B, C, P), dcenters (1, C, 1, J), dvariance (1, C, 1, J)) from the gradients of both outputs"""
    x, cen, s, d, q, S, qs, zp, n2, n, zn = (ctx[k] for k in ("x", "cen", "s", "d", "q", "S", "qs", "zp", "n2", "n", "zn"))
    C, J = cen.shape
    dzn = dz + torch.einsum("bci,bij->bcj", zn, dA + dA.transpose(1, 2))
    dot = (dzn * zn).sum(-1, keepdim=True)
    dzp = torch.where((n2 > EPS)[..., None], dzn - zn * dot, dzn) / n[..., None]
    sq = s * qs
    dS = dzp / sq
    dqs = -(dzp * S / (sq * qs)).sum(1)                                          # (B, J)
    dcen = -(dzp / s).sum(0)
    ds = -(dzp * zp / s).sum(0)
    dq = torch.einsum("bcp,bcj->bpj", x, dS) + dqs[:, None, :]
    dl = q * (dq - (q * dq).sum(-1, keepdim=True))
    dl = torch.where(d > EPS, dl, torch.zeros_like(dl))
    dx = torch.einsum("bpj,bcj->bcp", q, dS)
    for j in range(J):
        z = (x - cen[:, j, None]) / s[:, j, None]
        t = dl[:, None, :, j] * z / s[:, j, None]
        dx = dx - t
        dcen[:, j] += t.sum((0, 2))
        ds[:, j] += (t * z).sum((0, 2))
    dvar = ds * s * (1 - s)
    return dx, dcen.reshape(1, C, 1, J), dvar.reshape(1, C, 1, J)


class Pool(torch.autograd.Function):
    """(zn, A_out) = Pool.apply(x, centers, variance)"""

    @staticmethod
    def forward(c, x, centers, variance):
        zn, A, ctx = pool_forward(x, centers, variance)
        c.pool, c.shape = ctx, x.shape
        return zn, A

    @staticmethod
    def backward(c, dz, dA):
        dx, dcen, dvar = pool_backward(c.pool, dz, dA)
        return dx.reshape(c.shape), dcen, dvar


def literal(x, centers, variance):
    """the reference's call, line by line (materialises z for all vertices): small shapes only"""
    B, C = x.shape[0], x.shape[1]
    xr = x.reshape(B, C, -1, 1)
    z = (xr - centers) / torch.sigmoid(variance)
    q = torch.clamp((z * z).sum(1), min=EPS) * (-1 / 2)
    q = torch.softmax(q, -1)
    z = (q[:, None] * z).sum(-2)
    z = z / q.sum(-2, keepdim=True)
    z = z * torch.rsqrt(torch.clamp((z * z).sum(-1, keepdim=True), min=EPS))
    return z, torch.matmul(z.transpose(1, 2), z)


def glorot_limit(C, J):
    """Keras' glorot_uniform limit for a (1, C, 1, J) weight (sar_amd/stpgcn.py: glorot_uniform)"""
    return math.sqrt(6.0 / (C + J * C))


def make_case(regime, B, C, P, J, seed):
    """float64 (x (B, C, P), centers, variance) of the two input regimes: 'spread' (x = 0.3 relu(randn), centers 0.05 randn, variance
    0.5 randn) and 'init' (x = relu(randn), both parameters glorot-uniform: the ill-conditioned case, logits ~ -250 that differ by
    ~ 0.5)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda shape: torch.randn(shape, generator=g, dtype=torch.float64)
    if regime == "spread":
        return 0.3 * torch.relu(rn((B, C, P))), 0.05 * rn((1, C, 1, J)), 0.5 * rn((1, C, 1, J))
    assert regime == "init"
    lim = glorot_limit(C, J)
    u = lambda: (torch.rand(1, C, 1, J, generator=g, dtype=torch.float64) * 2 - 1) * lim
    return torch.relu(rn((B, C, P))), u(), u()


def preconditions(ctx):
    """(min qs, min d, min sum_j zp^2) of a float64 forward: the tests require >= 1e-3, > 1e-9, >= 1e-6"""
    return ctx["qs"].min().item(), ctx["d"].min().item(), ctx["n2"].min().item()
