"""Float64 restatement of the reference's models/stgcn_debug.py `Model` (a helper, not a test): ST-GCN built from oracle/stgcn.py's
own pieces -- data_bn, batch_norm, temporal_conv, the residual kinds, _relu with prescribed masks, loss_fn -- with ONE change: the
graph contraction of every block is SGTACN's einsum 'nkctv,ktvw->nctw' with the block's own table `l{i}.adjacency_matrix` of shape
(K, T_i, V, V) (models/stgcn_debug.py:118-145), a differentiable leaf."""
import torch
import torch.nn.functional as F

from oracle import stgcn as O


def table_name(i):
    return "l%d.adjacency_matrix" % i


def block_frames(frames, blocks=None):
    """input frame count of every block"""
    out, T = [], int(frames)
    for f, s, res in (blocks or O.BLOCKS):
        out.append(T)
        T = O.same_pad(T, O.KT, s)[0]
    return out


def init_tables(p, frames, blocks=None):
    """adds the tables to an oracle parameter dict: p['A'] repeated over every block's input frames (stgcn_debug.py:129-132)"""
    A = p["A"]
    for i, T in enumerate(block_frames(frames, blocks)):
        p[table_name(i)] = A.unsqueeze(1).repeat(1, T, 1, 1).clone()
    return p


def is_trainable(name):
    return O.is_trainable(name)       # (the tables are trainable: only 'A' and the moving statistics are not)


def graph_conv_ta(x, kernel, bias, At):
    """models/stgcn_debug.py:135-145.  x (B, Cin, T, V); kernel (1, 1, Cin, K F); At (K, T, V, V)."""
    y = F.conv2d(x, O.hwio_to_oihw(kernel), bias)
    B, KF, T, V = y.shape
    K = At.shape[0]
    return torch.einsum("nkctv,ktvw->nctw", y.reshape(B, K, KF // K, T, V), At)


def st_block(x, p, i, training, new_stats=None, taps=None, blocks=None, masks=None):
    """oracle.stgcn.st_block with the contraction replaced (models/stgcn_debug.py:216-222)"""
    f, s, res = (blocks or O.BLOCKS)[i]
    pre = "l%d." % i
    kind = O.block_residual_kind(x.shape[1], f, s, res)
    if kind == "none":
        r = None
    elif kind == "identity":
        r = x
    else:
        r = F.conv2d(x, O.hwio_to_oihw(p[pre + "res.kernel"]), p[pre + "res.bias"], stride=(s, 1))
        r = O.batch_norm(r, p[pre + "res_bn.gamma"], p[pre + "res_bn.beta"], p[pre + "res_bn.moving_mean"],
                         p[pre + "res_bn.moving_var"], training, (0, 2, 3), True, new_stats, pre + "res_bn")
    g = graph_conv_ta(x, p[pre + "gcn.kernel"], p[pre + "gcn.bias"], p[table_name(i)])
    h = O.batch_norm(g, p[pre + "bn1.gamma"], p[pre + "bn1.beta"], p[pre + "bn1.moving_mean"], p[pre + "bn1.moving_var"], training,
                     (0, 2, 3), True, new_stats, pre + "bn1")
    h = O._relu(h, masks, pre + "h")
    u = O.temporal_conv(h, p[pre + "tcn.kernel"], p[pre + "tcn.bias"], s)
    z = O.batch_norm(u, p[pre + "bn2.gamma"], p[pre + "bn2.beta"], p[pre + "bn2.moving_mean"], p[pre + "bn2.moving_var"], training,
                     (0, 2, 3), True, new_stats, pre + "bn2")
    if r is not None:
        z = z + r
    y = O._relu(z, masks, pre + "y")
    if taps is not None:
        taps[pre + "g"], taps[pre + "u"], taps[pre + "y"] = g, u, y
    return y


def forward(p, x, training, new_stats=None, taps=None, blocks=None, masks=None):
    """models/stgcn_debug.py:269-293.  x (N, C, T, V, M) -> logits (N, classes)."""
    N, C, T, V, M = x.shape
    h = O.data_bn(x, p, training, new_stats)
    for i in range(len(blocks or O.BLOCKS)):
        h = st_block(h, p, i, training, new_stats, taps, blocks, masks)
    feat = h.mean(dim=(2, 3)).reshape(N, M, -1).mean(dim=1)
    return feat @ p["logits.kernel"][0, 0] + p["logits.bias"]


def loss_and_grads(p, x, labels, global_batch_size=None, blocks=None, masks=None):
    """one train step's differentiable part: every trainable variable, the tables included"""
    names = [k for k in p if is_trainable(k)]
    leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
    q = dict(p)
    q.update(leaves)
    new_stats, taps = {}, {}
    logits = forward(q, x, True, new_stats, taps, blocks, masks)
    loss = O.loss_fn(logits, labels, global_batch_size or x.shape[0])
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return logits.detach(), loss.detach(), dict(zip(names, grads)), new_stats, {k: v.detach() for k, v in taps.items()}
