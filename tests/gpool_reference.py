"""Restatement of the reference's GPool (models/stgcn_debug.py:29-72) and SGCN (:93-115) in torch ops, in the dtype of its inputs:
the forward line by line, and the backward written by hand from the formulas the kernels of csrc/gpool.hip implement (tests/
test_gpool_reference.py holds it against autograd of the literal forward).  No gradient passes through the selection."""
import math

import numpy as np
import torch

EPS = 1e-12


def keep_of(keeprate, V):
    """int(keeprate * tf.cast(V, float32)): the product is formed in float32, then truncated"""
    keep = int(np.float32(keeprate) * np.float32(V))
    if not (0.0 < float(keeprate) <= 1.0) or keep < 1:
        raise ValueError("keeprate %r keeps %d of %d vertices" % (keeprate, keep, V))
    return keep


def argsort_desc(y):
    """tf.argsort(DESCENDING, stable): equal scores in ascending index; a NaN ranks below every number"""
    key = torch.where(torch.isnan(y), torch.full_like(y, -math.inf), y)
    order = torch.argsort(key, dim=1, descending=True, stable=True)
    nan_last = torch.argsort(torch.isnan(y).gather(1, order).to(torch.int8), dim=1, stable=True)
    return order.gather(1, nan_last)


def forward(x, A, p, keeprate):
    """x (N, C, T, V), A (N, K, V, V), p (C T, 1) -> out (N, C, T, keep), A_out (N, K, keep, keep), y (N, V), idx (N, keep)"""
    N, C, T, V = x.shape
    K = A.shape[1]
    xr = x.reshape(N, C * T, V).transpose(1, 2)                                        # (N, V, C T)
    ph = p / torch.sqrt(torch.clamp((p * p).sum(), min=EPS))                            # tf.math.l2_normalize
    y = (xr @ ph)[..., 0]
    keep = keep_of(keeprate, V)
    idx = argsort_desc(y.detach())[:, :keep]
    s = torch.sigmoid(torch.gather(y, 1, idx))
    xg = torch.gather(xr, 1, idx[:, :, None].expand(-1, -1, C * T)) * s[:, :, None]
    A2 = A @ A
    rows = torch.gather(A2, 2, idx[:, None, :, None].expand(-1, K, -1, V))
    A_out = torch.gather(rows, 3, idx[:, None, None, :].expand(-1, K, keep, -1))
    return xg.transpose(1, 2).reshape(N, C, T, keep), A_out, y, idx


def backward(x, A, p, idx, y, dout, dA_out):
    """(dx, dp, dA) by hand; dout or dA_out may be None (its gradients are then None)"""
    N, C, T, V = x.shape
    keep = idx.shape[1]
    dx = dp = dA = None
    if dout is not None:
        n2 = (p * p).sum()
        nrm = torch.sqrt(torch.clamp(n2, min=EPS))
        ph = (p / nrm)[:, 0]
        xr, do = x.reshape(N, C * T, V), dout.reshape(N, C * T, keep)
        sel = idx[:, None, :].expand(-1, C * T, -1)
        xs = torch.gather(xr, 2, sel)
        s = torch.sigmoid(torch.gather(y, 1, idx))
        ds = (do * xs).sum(1)
        dy_sel = ds * s * (1 - s)
        dy = torch.zeros_like(y).scatter(1, idx, dy_sel)
        dx = (torch.zeros_like(xr).scatter(2, sel, do * s[:, None, :]) + dy[:, None, :] * ph[None, :, None]).reshape(x.shape)
        dph = torch.einsum("ni,nci->c", dy_sel, xs)
        dp = (((dph - ph * (dph * ph).sum()) / nrm) if bool(n2 > EPS) else dph / nrm)[:, None]
    if dA_out is not None:
        G = torch.zeros_like(A)
        for n in range(N):
            G[n][:, idx[n][:, None], idx[n][None, :]] = dA_out[n]
        dA = G @ A.transpose(2, 3) + A.transpose(2, 3) @ G
    return dx, dp, dA


def make_case(shape, seed, dtype=torch.float64):
    """x = relu(randn), p glorot uniform, A sparse non-negative, random dout and dA_out"""
    N, C, T, V, K, keeprate = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, C, T, V, generator=g, dtype=torch.float64))
    lim = math.sqrt(6.0 / (C * T + 1))
    p = (torch.rand(C * T, 1, generator=g, dtype=torch.float64) * 2 - 1) * lim
    A = torch.rand(N, K, V, V, generator=g, dtype=torch.float64) * (torch.rand(N, K, V, V, generator=g) < 0.3)
    keep = keep_of(keeprate, V)
    dout = torch.randn(N, C, T, keep, generator=g, dtype=torch.float64)
    dA_out = torch.randn(N, K, keep, keep, generator=g, dtype=torch.float64)
    return tuple(t.to(dtype) for t in (x, A, p, dout, dA_out))


def min_gap(y):
    """the smallest difference of consecutive sorted scores of a sample, relative to max |y| (inf for one vertex)"""
    if y.shape[1] < 2:
        return math.inf
    ys = torch.sort(y.double(), dim=1, descending=True)[0]
    return ((ys[:, :-1] - ys[:, 1:]).min() / y.double().abs().max()).item()


def sgcn_forward(x, A, kernel, bias):
    """Conv2D(K F, 1x1) with the Keras kernel (1, 1, C, K F) (channel k F + m), then einsum 'nkctv,nkvw->nctw'; written with matmul"""
    N, C, T, V = x.shape
    K = A.shape[1]
    F = kernel.shape[-1] // K
    W = kernel.reshape(C, K, F)
    out = torch.zeros(N, F, T, V, dtype=x.dtype)
    for k in range(K):
        yk = (x.permute(0, 2, 3, 1) @ W[:, k, :] + bias[k * F:(k + 1) * F]).permute(0, 3, 1, 2)     # (N, F, T, V)
        out = out + yk @ A[:, k][:, None]
    return out
