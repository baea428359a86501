"""Float64 torch restatements of the reference's two graph isomorphism layers, written from the text of models/gcn.py:54-163 (the
reference is TensorFlow and does not run here), in the style of tests/gcn_reference.py:

  GraphIsoConv    models/gcn.py:54-93    A_ = A + diag(1 + epsilon);  x = einsum('ncv,nvw->ncw', x, A_);  x = mlp(x)
  GraphIsoConvTD  models/gcn.py:112-163  A_ = concat(A, diag(1 + epsilon)[None]);  x = einsum('nctv,kvw->nkctw', x, A_);
                                         x = sum_k mlps[k](x[:, k])

An MLP over `filters` is Conv(f, 1) -> BatchNormalization(axis=1) -> ReLU per entry; with return_logits the last entry is the bare
convolution.  Parameters are read from a dict with the layers' state_dict names (`epsilon`, `mlp.{i}.kernel` (1, Cin, f) ..,
`mlps.{k}.{i}.kernel` (1, 1, Cin, f) ..).  BatchNormalization: eps 1e-3, momentum 0.99; the statistics run over every axis but 1;
the moving variance takes the biased batch variance on the 3-D input of GraphIsoConv (Keras' non-fused path) and the unbiased one on
the 4-D input of GraphIsoConvTD (the fused path), SURVEY.md 8(c)."""
import torch

BN_EPS, BN_MOMENTUM = 1e-3, 0.99


def _batch_norm(a, p, q, training, unbiased_moving, new_stats):
    axes = [0] + list(range(2, a.dim()))
    shape = [1, -1] + [1] * (a.dim() - 2)
    if training:
        mean, var = a.mean(dim=axes), a.var(dim=axes, unbiased=False)
        if new_stats is not None:
            n = a.numel() // a.shape[1]
            v_mov = var * (n / (n - 1)) if unbiased_moving else var
            new_stats[q + "moving_mean"] = p[q + "moving_mean"] * BN_MOMENTUM + mean.detach() * (1 - BN_MOMENTUM)
            new_stats[q + "moving_var"] = p[q + "moving_var"] * BN_MOMENTUM + v_mov.detach() * (1 - BN_MOMENTUM)
    else:
        mean, var = p[q + "moving_mean"], p[q + "moving_var"]
    return (a - mean.view(shape)) * (torch.rsqrt(var + BN_EPS) * p[q + "gamma"]).view(shape) + p[q + "beta"].view(shape)


def _mlp(a, p, pre, filters, return_logits, training, unbiased_moving, new_stats, pre_relu):
    """a (N, C, ...) through Conv(f, 1) [-> BN -> ReLU] per entry of `filters`; kernels (1, .., 1, Cin, f)"""
    for i in range(len(filters)):
        q = "%s%d." % (pre, i)
        kernel = p[q + "kernel"]
        w = kernel.reshape(kernel.shape[-2], kernel.shape[-1])
        a = torch.einsum("nc...,cf->nf...", a, w) + p[q + "bias"].view([1, -1] + [1] * (a.dim() - 2))
        if i < len(filters) - 1 or not return_logits:
            a = _batch_norm(a, p, q, training, unbiased_moving, new_stats)
            if pre_relu is not None:
                pre_relu.append(a)
            a = torch.relu(a)
    return a


def graph_iso_conv(x, A, p, filters, return_logits=False, training=True, new_stats=None, pre_relu=None):
    """x (N, C, V), A (N, V, V) -> (N, filters[-1], V)"""
    V = A.shape[-1]
    A_ = A + torch.diag(torch.ones(V, dtype=x.dtype) + p["epsilon"])
    a = torch.einsum("ncv,nvw->ncw", x, A_)
    return _mlp(a, p, "mlp.", filters, return_logits, training, False, new_stats, pre_relu)


def graph_iso_conv_td(x, A, p, filters, kernel_size=3, return_logits=False, training=True, new_stats=None, pre_relu=None):
    """x (B, C, T, V), A (kernel_size - 1, V, V) -> (B, filters[-1], T, V)"""
    V = A.shape[-1]
    self_connections = torch.diag(torch.ones(V, dtype=x.dtype) + p["epsilon"]).unsqueeze(0)
    A_ = torch.cat([A, self_connections], dim=0)
    assert A_.shape[0] == kernel_size
    z = torch.einsum("nctv,kvw->nkctw", x, A_)
    out = 0
    for k in range(kernel_size):
        out = out + _mlp(z[:, k], p, "mlps.%d." % k, filters, return_logits, training, True, new_stats, pre_relu)
    return out


def init_params(filters, in_channels, kernel_size=None, return_logits=False, seed=0):
    """random float64 parameters with the layers' names: kernel_size None = GraphIsoConv, else GraphIsoConvTD"""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    p = {"epsilon": 0.3 + 0.1 * rnd(())}
    for pre, lead in ([("mlp.", (1,))] if kernel_size is None else [("mlps.%d." % k, (1, 1)) for k in range(kernel_size)]):
        cin = in_channels
        for i, f in enumerate(filters):
            q = "%s%d." % (pre, i)
            p[q + "kernel"], p[q + "bias"] = rnd(*lead, cin, f) / cin ** 0.5, 0.2 * rnd(f)
            if i < len(filters) - 1 or not return_logits:
                p[q + "gamma"], p[q + "beta"] = 1 + 0.2 * rnd(f), 0.2 * rnd(f)
                p[q + "moving_mean"], p[q + "moving_var"] = 0.1 * rnd(f), 1 + 0.1 * rnd(f).abs()
            cin = f
    return p


def layer_params(layer):
    """a layer's own parameters and moving statistics as the float64 dict the restatements read"""
    return {k: v.detach().double().cpu() for k, v in layer.state_dict().items()}


def to_oracle(p, pre="l0."):
    """GraphIsoConvTD parameters for filters = [h, h] under the names oracle.stgin.graph_iso_conv reads for block `pre`"""
    out = {pre + "epsilon": p["epsilon"]}
    for k, v in p.items():
        if k.startswith("mlps."):
            _, br, i, part = k.split(".")
            if part in ("kernel", "bias"):
                out["%smlp%s.c%d.%s" % (pre, br, int(i) + 1, part)] = v
            else:
                out["%smlp%s.bn%d.%s" % (pre, br, int(i) + 1, part)] = v
    return out
