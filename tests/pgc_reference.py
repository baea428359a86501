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
    ctx = dict(x=x, cen=cen, s=s, d=d, q=q, S=S_, qs=qs, shape=shape)
    ctx.update(pgc_graph(S_, qs, cen, s, kernel[0], bias))
    out = x + torch.einsum("bpj,bfj->bfp", q, ctx["h"])
    return out.reshape(shape), ctx


def pgc_graph(S_, qs, cen, s, W, bias):
    """the per-sample part of the forward pass, from S = x q^T (B, C, J) and qs = sum_p q (B, 1, J): the projected graph and its
    convolution (one kernel of csrc/pgc.hip: tests/test_gpu_pgc_edges.py calls this on the sums it hands that kernel)"""
    zp = (S_ - cen * qs) / (s * qs)
    n2 = (zp * zp).sum(-1)
    n = torch.sqrt(torch.clamp(n2, min=EPS))
    zn = zp / n[..., None]
    A = torch.einsum("bci,bcj->bij", zn, zn)
    g = torch.einsum("cf,bcj->bfj", W, zn) + bias[None, :, None]
    h = torch.einsum("bfi,bij->bfj", g, A)
    return dict(zp=zp, n2=n2, n=n, zn=zn, A=A, W=W, g=g, h=h)


def pgc_graph_backward(c, dh):
    """the per-sample part of the backward pass, from dh = dout q^T (B, F, J) and what pgc_graph made (c: S, qs, s, zp, n2, zn, A, W,
    g).  -> dict: dS, dqs (B, J), the pooled-path terms of dcenters / ds per sample, dW (B, C, F) and dbias (B, F) per sample"""
    S_, qs, s, zp, n2, zn, A, W, g = (c[k] for k in ("S", "qs", "s", "zp", "n2", "zn", "A", "W", "g"))
    n = torch.sqrt(torch.clamp(n2, min=EPS))
    dg = torch.einsum("bfj,bij->bfi", dh, A)
    dA = torch.einsum("bfi,bfj->bij", g, dh)
    dzn = torch.einsum("cf,bfj->bcj", W, dg) + torch.einsum("bci,bij->bcj", zn, dA + dA.transpose(1, 2))
    dot = (dzn * zn).sum(-1, keepdim=True)
    dzp = torch.where((n2 > EPS)[..., None], dzn - zn * dot, dzn) / n[..., None]
    sq = s * qs
    # (dzp / sq) (S / qs) and not dzp S / (sq qs): s qs^2 underflows in float32 for a vertex that takes almost no column (qs below
    # 1e-19) while both quotients stay finite
    dqs = -((dzp / sq) * (S_ / qs)).sum(1)                                       # (B, J)
    return dict(dS=dzp / sq, dqs=dqs, pool_c=-(dzp / s), pool_s=-(dzp * zp / s), dW=torch.einsum("bcj,bfj->bcf", zn, dg), dbias=dg.sum(2))


def pgc_column_backward(x, dout, q, h, dS, dqs, cen, s):
    """the per-column part of the backward pass -> dict: dx (B, C, P), dl (B, P, J) and dl_free (dl without the clamp's zeros), the
    per-sample column sums col_c = sum_p dl z and col_s = sum_p dl z^2 (B, C, J)"""
    J = cen.shape[1]
    d = torch.stack([(((x - cen[:, j, None]) / s[:, j, None]) ** 2).sum(1) for j in range(J)], -1)
    dq = torch.einsum("bcp,bcj->bpj", dout, h) + torch.einsum("bcp,bcj->bpj", x, dS) + dqs[:, None, :]
    dl_free = q * (dq - (q * dq).sum(-1, keepdim=True))
    dl = torch.where(d > EPS, dl_free, torch.zeros_like(dl_free))
    dx = dout + torch.einsum("bpj,bcj->bcp", q, dS)
    col_c, col_s = torch.zeros_like(dS), torch.zeros_like(dS)
    for j in range(J):
        z = (x - cen[:, j, None]) / s[:, j, None]
        t = dl[:, None, :, j] * z
        dx = dx - t / s[:, j, None]
        col_c[:, :, j] = t.sum(2)
        col_s[:, :, j] = (t * z).sum(2)
    return dict(dx=dx, dl=dl, dl_free=dl_free, col_c=col_c, col_s=col_s)


def pgc_param_grad(col_c, col_s, pool_c, pool_s, s):
    """sums over the batch (C, J) -> (dcenters, dvariance)"""
    ds = pool_s + col_s / s
    return pool_c + col_c / s, ds * s * (1 - s)


def pgc_backward(ctx, dout, taps=None):
    """-> (dx like x, dcenters, dvariance, dkernel, dbias).  taps (a dict) gains what each kernel of csrc/pgc.hip hands to the next, per
    sample (dh and the results of pgc_graph_backward and pgc_column_backward)."""
    x, cen, s, q = (ctx[k] for k in ("x", "cen", "s", "q"))
    B, C = x.shape[:2]
    dout = dout.reshape(B, C, -1)
    dh = torch.einsum("bfp,bpj->bfj", dout, q)
    gb = pgc_graph_backward(ctx, dh)
    cb = pgc_column_backward(x, dout, q, ctx["h"], gb["dS"], gb["dqs"], cen, s)
    dcen, dvar = pgc_param_grad(cb["col_c"].sum(0), cb["col_s"].sum(0), gb["pool_c"].sum(0), gb["pool_s"].sum(0), s)
    if taps is not None:
        taps.update(gb, dh=dh, **{k: v for k, v in cb.items() if k != "dx"})
    J = cen.shape[1]
    return cb["dx"].reshape(ctx["shape"]), dcen.reshape(1, C, 1, J), dvar.reshape(1, C, 1, J), gb["dW"].sum(0)[None], gb["dbias"].sum(0)


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
