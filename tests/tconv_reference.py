"""The float64 restatement of TemporalConv (csrc/tconv.hip, models/tcn.py), written from the definition and from nothing else:

  out[n,m,to,v] = bias[m] + sum_{j<k} sum_c W[j,c,m] x[n, c, to s + j d - pad, v]                     (x is 0 outside [0, T))
  dx [n,c,u,v]  = sum_j sum_m W[j,c,m] dout[n, m, (u + pad - j d) / s, v]                             (exact quotients in [0, T_out) only)
  dW [j,c,m]    = sum_{n,to,v} x[n, c, to s + j d - pad, v] dout[n,m,to,v]        dbias[m] = sum_{n,to,v} dout[n,m,to,v]

One explicit gather over (to, j): every (output frame, tap) pair that meets a real frame contributes one (N, C, V) x (C, M) product; the
gradients walk the same pairs.  W is the Keras kernel (k, 1, C, M).  Runs in the dtype of its inputs (the float32 run gives the band of
tests/test_gpu_tconv.py).  A helper of the tconv tests, not a test."""
import torch


def geometry(T, k, s, d, padding):
    """(T_out, pad): padding="same" is TensorFlow's SAME with the dilated extent (the odd frame of padding goes behind), an int p is
    PyTorch's symmetric padding"""
    if padding == "same":
        T_out = (T + s - 1) // s
        total = max((T_out - 1) * s + (k - 1) * d + 1 - T, 0)
        return T_out, total // 2
    return (T + 2 * padding - d * (k - 1) - 1) // s + 1, padding


def pairs(T, T_out, k, s, d, pad):
    """the (to, j, t) with t = to s + j d - pad a real frame"""
    return [(to, j, to * s + j * d - pad) for to in range(T_out) for j in range(k) if 0 <= to * s + j * d - pad < T]


def forward(x, W, bias, s, d, pad, T_out):
    N, C, T, V = x.shape
    k, _, _, M = W.shape
    out = torch.zeros((N, M, T_out, V), dtype=x.dtype)
    for to, j, t in pairs(T, T_out, k, s, d, pad):
        out[:, :, to, :] += torch.einsum("ncv,cm->nmv", x[:, :, t, :], W[j, 0])
    if bias is not None:
        out += bias.view(1, M, 1, 1)
    return out


def backward(x, W, dout, s, d, pad):
    """(dx, dW (k, 1, C, M), dbias (M))"""
    N, C, T, V = x.shape
    k, _, _, M = W.shape
    T_out = dout.shape[2]
    dx, dW = torch.zeros_like(x), torch.zeros_like(W)
    for to, j, t in pairs(T, T_out, k, s, d, pad):
        dx[:, :, t, :] += torch.einsum("nmv,cm->ncv", dout[:, :, to, :], W[j, 0])
        dW[j, 0] += torch.einsum("ncv,nmv->cm", x[:, :, t, :], dout[:, :, to, :])
    return dx, dW, dout.sum(dim=(0, 2, 3))
