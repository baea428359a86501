"""Float64 torch restatements of the reference's layer classes that the oracle does not hold, written from the text of
models/gcn.py (the reference is TensorFlow and does not run here):

  GraphConv     models/gcn.py:22-36    x = Conv1D(filters, 1, channels_first)(x);  x = einsum('ncv,nvw->ncw', x, A)
  AdjGraphConv  models/gcn.py:212-238  x = Conv2D(K filters, 1, channels_first)(x); reshape (N, K, filters, T, V);
                                       x = einsum('nkctv,kvw->nctw', x, A) with A the layer's trainable variable

Kernels are in the Keras layouts: Conv1D (1, C, filters), Conv2D (1, 1, C, K filters); the Conv2D's output channel k * filters + m is
slice k, filter m (the reshape above splits the channel axis with K outermost).  GraphConvTD and the ST-GCN block are checked
against oracle.stgcn.graph_conv_td / st_block, the block fed the layer's own parameters through block_params."""
import torch


def graph_conv(x, A, kernel, bias):
    """x (N, C, V), A (N, V, V), kernel (1, C, F), bias (F) -> (N, F, V)"""
    y = torch.einsum("ncv,cf->nfv", x, kernel[0]) + bias.view(1, -1, 1)
    return torch.einsum("ncv,nvw->ncw", y, A)


def adj_graph_conv(x, A, kernel, bias):
    """x (B, C, T, V), A (K, V, V), kernel (1, 1, C, K F), bias (K F) -> (B, F, T, V)"""
    y = torch.einsum("nctv,cf->nftv", x, kernel[0, 0]) + bias.view(1, -1, 1, 1)
    N, KF, T, V = y.shape
    K = A.shape[0]
    return torch.einsum("nkctv,kvw->nctw", y.reshape(N, K, KF // K, T, V), A)


def oracle_name(k):
    """a SpatioTemporalGraphConv state_dict key -> the oracle's name for block 0: sgcn.kernel -> l0.gcn.kernel, bn1_gamma -> l0.bn1.gamma,
    res_bn_moving_var -> l0.res_bn.moving_var"""
    if k.startswith("sgcn."):
        return "l0.gcn." + k[5:]
    for tail in ("moving_mean", "moving_var", "gamma", "beta", "kernel", "bias"):
        if k.endswith("_" + tail):
            return "l0.%s.%s" % (k[:-len(tail) - 1], tail)
    raise KeyError(k)


def block_params(layer):
    """a SpatioTemporalGraphConv's own parameters and moving statistics as the float64 dict oracle.stgcn.st_block reads for block 0"""
    return {oracle_name(k): v.detach().double().cpu() for k, v in layer.state_dict().items()}
