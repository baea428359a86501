"""Float64 restatement of ProjectionGraphConv(64, 32) (the reference's models/stpgcn.py:11-47 with GraphConv models/gcn.py:22-37)
and of the ST-PGCN network built from oracle/stgcn.py's pieces, for the tests of sar_amd/stpgcn.py.

pgc_forward / pgc_backward: the layer with a hand-written backward pass (pinned by central finite differences in
tests/test_pgc_reference.py).  The per-column distances are formed one vertex at a time, so that z = (x - centers) / s is never held
for all 32 vertices at once.  PGC wraps the pair as an autograd function; forward / loss_and_grads are oracle.stgcn's with the layer
after block 0 (models/stpgcn.py:141-152)."""
import torch

from oracle import stgcn as S

EPS = 1e-12
NAMES = ("pgc.centers", "pgc.variance", "pgc.gcn.kernel", "pgc.gcn.bias")


def pgc_forward(x, centers, variance, kernel, bias):
    """x (B, C, T, V) or (B, C, P); centers / variance (1, C, 1, J); kernel (1, C, F); bias (F,).  Returns (out like x, ctx)."""
    shape = x.shape
    B, C = shape[0], shape[1]
    x = x.reshape(B, C, -1)
    cen, s = centers.reshape(C, -1), torch.sigmoid(variance.reshape(C, -1))
    J = cen.shape[1]
    d = torch.stack([(((x - cen[:, j, None]) / s[:, j, None]) ** 2).sum(1) for j in range(J)], -1)     # (B, P, J)
    q = torch.softmax(torch.clamp(d, min=EPS) * -0.5, -1)
    S_ = torch.einsum("bcp,bpj->bcj", x, q)
    qs = q.sum(1)[:, None, :]
    zp = (S_ - cen * qs) / (s * qs)
    n2 = (zp * zp).sum(-1)
    n = torch.sqrt(torch.clamp(n2, min=EPS))
    zn = zp / n[..., None]
    A = torch.einsum("bci,bcj->bij", zn, zn)
    W = kernel[0]
    g = torch.einsum("cf,bcj->bfj", W, zn) + bias[None, :, None]
    h = torch.einsum("bfi,bij->bfj", g, A)
    out = x + torch.einsum("bpj,bfj->bfp", q, h)
    ctx = dict(x=x, cen=cen, s=s, d=d, q=q, S=S_, qs=qs, zp=zp, n2=n2, n=n, zn=zn, A=A, W=W, g=g, h=h, shape=shape)
    return out.reshape(shape), ctx


def pgc_backward(ctx, dout):
    """-> (dx like x, dcenters, dvariance, dkernel, dbias)"""
    x, cen, s, d, q, S_, qs, zp, n2, n, zn, A, W, g, h = (ctx[k] for k in ("x", "cen", "s", "d", "q", "S", "qs", "zp", "n2", "n", "zn",
                                                                              "A", "W", "g", "h"))
    B, C = x.shape[:2]
    dout = dout.reshape(B, C, -1)
    dh = torch.einsum("bfp,bpj->bfj", dout, q)
    dg = torch.einsum("bfj,bij->bfi", dh, A)
    dA = torch.einsum("bfi,bfj->bij", g, dh)
    dW = torch.einsum("bcj,bfj->cf", zn, dg)
    dbias = dg.sum((0, 2))
    dzn = torch.einsum("cf,bfj->bcj", W, dg) + torch.einsum("bci,bij->bcj", zn, dA + dA.transpose(1, 2))
    dot = (dzn * zn).sum(-1, keepdim=True)
    dzp = torch.where((n2 > EPS)[..., None], dzn - zn * dot, dzn) / n[..., None]
    sq = s * qs
    dS = dzp / sq
    dqs = -(dzp * S_ / (sq * qs)).sum(1)                                         # (B, J)
    dcen = -(dzp / s).sum(0)
    ds = -(dzp * zp / s).sum(0)
    dq = torch.einsum("bcp,bcj->bpj", dout, h) + torch.einsum("bcp,bcj->bpj", x, dS) + dqs[:, None, :]
    dl = q * (dq - (q * dq).sum(-1, keepdim=True))
    dl = torch.where(d > EPS, dl, torch.zeros_like(dl))
    dx = dout + torch.einsum("bpj,bcj->bcp", q, dS)
    for j in range(cen.shape[1]):
        z = (x - cen[:, j, None]) / s[:, j, None]
        t = dl[:, None, :, j] * z / s[:, j, None]
        dx = dx - t
        dcen[:, j] += t.sum((0, 2))
        ds[:, j] += (t * z).sum((0, 2))
    dvar = ds * s * (1 - s)
    J = cen.shape[1]
    return dx.reshape(ctx["shape"]), dcen.reshape(1, C, 1, J), dvar.reshape(1, C, 1, J), dW[None], dbias


class PGC(torch.autograd.Function):
    @staticmethod
    def forward(c, x, centers, variance, kernel, bias):
        out, ctx = pgc_forward(x, centers, variance, kernel, bias)
        c.pgc = ctx
        return out

    @staticmethod
    def backward(c, dout):
        return pgc_backward(c.pgc, dout)


def init_pgc(p, seed, dtype=torch.float64, scale=1.0):
    """p gains the four layer parameters (random, layer-sized draws: tests)"""
    g = torch.Generator().manual_seed(seed)
    p["pgc.centers"] = (0.5 * scale * torch.randn(1, 64, 1, 32, generator=g)).to(dtype)
    p["pgc.variance"] = (0.5 * torch.randn(1, 64, 1, 32, generator=g)).to(dtype)
    p["pgc.gcn.kernel"] = (0.2 * torch.randn(1, 64, 64, generator=g)).to(dtype)
    p["pgc.gcn.bias"] = (0.1 * torch.randn(64, generator=g)).to(dtype)
    return p


def forward(p, x, training, new_stats=None, taps=None, blocks=None, masks=None):
    """oracle.stgcn.forward with the layer after block 0"""
    N, C, T, V, M = x.shape
    h = S.data_bn(x, p, training, new_stats)
    if taps is not None:
        taps["x0"] = h
    for i in range(len(blocks or S.BLOCKS)):
        h = S.st_block(h, p, i, p["A"], training, new_stats, taps, blocks, masks)
        if i == 0:
            h = PGC.apply(h, *(p[k] for k in NAMES))
            if taps is not None:
                taps["pgc.out"] = h
    pooled = h.mean(dim=(2, 3))
    feat = pooled.reshape(N, M, -1).mean(dim=1)
    return feat @ p["logits.kernel"][0, 0] + p["logits.bias"]


def loss_and_grads(p, x, labels, global_batch_size=None, blocks=None, masks=None):
    names = S.trainable_names(p)
    leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
    q = dict(p)
    q.update(leaves)
    new_stats, taps = {}, {}
    logits = forward(q, x, True, new_stats, taps, blocks, masks)
    loss = S.loss_fn(logits, labels, global_batch_size or x.shape[0])
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return logits.detach(), loss.detach(), dict(zip(names, grads)), new_stats, {k: v.detach() for k, v in taps.items()}
