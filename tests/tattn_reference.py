"""TemporalAttention(num_hidden) (reference models/stgcn.py:67-85) restated in torch with a hand-written backward; runs in the dtype
of its inputs (float64 = the oracle of tests/test_gpu_tattn.py, the same code in float32 = its band).

    f[r, v C + c] = x[n, c, t, v]   (r = n T + t; the reference transposes to (N, T, V, C) before its reshape)      h_0 = f
    z_i = h_{i-1} kernel_i + bias_i         h_i = relu(z_i) (i < L)         a[n, t] = sigmoid(z_L)
    out[n, c, t, v] = x[n, c, t, v] a[n, t]

    da[r] = sum_{c,v} dout x       dz_L = da a (1 - a)
    dkernel_i = h_{i-1}^T dz_i     dbias_i = sum_r dz_i     dh_{i-1} = dz_i kernel_i^T     dz_i = dh_i [h_i > 0]  (0 at 0, as TensorFlow)
    dx = dout a + unflatten(dz_1 kernel_1^T)

params = [kernel_1, bias_1, .., kernel_L, bias_L], Keras layouts: kernel (in, units), bias (units); units_L = 1."""
import torch


def features(x):
    N, C, T, V = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * T, V * C)


def forward(x, params):
    """-> (out, ctx); ctx holds x, params, hs = [f, h_1, .., h_L] (rows r), zs = [z_1, .., z_L] and a (N, T)"""
    N, C, T, V = x.shape
    nl = len(params) // 2
    hs, zs = [features(x)], []
    for i in range(nl):
        z = hs[-1] @ params[2 * i] + params[2 * i + 1]
        zs.append(z)
        hs.append(torch.sigmoid(z) if i == nl - 1 else torch.relu(z))
    a = hs[-1].reshape(N, T)
    return x * a.view(N, 1, T, 1), dict(x=x, params=list(params), hs=hs, zs=zs, a=a)


def backward(ctx, dout, need_dx=True):
    """-> (dx | None, grads in the order of params, dzs = [dz_1, .., dz_L] (rows r))"""
    x, params, hs, a = ctx["x"], ctx["params"], ctx["hs"], ctx["a"]
    N, C, T, V = x.shape
    nl = len(params) // 2
    da = (dout * x).sum(dim=(1, 3)).reshape(N * T, 1)
    av = a.reshape(N * T, 1)
    dz = da * av * (1 - av)
    grads, dzs = [None] * len(params), [None] * nl
    for i in range(nl - 1, -1, -1):
        dzs[i] = dz
        grads[2 * i], grads[2 * i + 1] = hs[i].t() @ dz, dz.sum(dim=0)
        if i > 0 or need_dx:
            dh = dz @ params[2 * i].t()
        if i > 0:
            dz = dh * (hs[i] > 0).to(dh.dtype)
    dx = dout * a.view(N, 1, T, 1) + dh.reshape(N, T, V, C).permute(0, 3, 1, 2) if need_dx else None
    return dx, grads, dzs


def literal(x, params):
    """the reference's call, line by line, in torch ops (for autograd): transpose, reshape, Dense .., multiply, transpose back"""
    N, C, T, V = x.shape
    nl = len(params) // 2
    xt = x.permute(0, 2, 3, 1)                                                         # tf.transpose(x, [0, 2, 3, 1])
    h = xt.reshape(-1, T, V * C)                                                       # tf.reshape(x, [-1, T, V * C])
    for i in range(nl):
        h = torch.nn.functional.linear(h, params[2 * i].t(), params[2 * i + 1])       # Dense: h kernel + bias
        h = torch.sigmoid(h) if i == nl - 1 else torch.relu(h)
    xt = xt * h.reshape(N, T, 1, 1)                                                    # tf.math.multiply(x, tf.reshape(attention, [N, T, 1, 1]))
    return xt.permute(0, 3, 1, 2)                                                      # tf.transpose(x, [0, 3, 1, 2])


def relu_margins(ctx):
    """per hidden layer: min |z| / rms(z) -- how far the nearest pre-activation is from the ReLU's kink, in units of the layer's RMS"""
    return [(z.abs().min() / z.pow(2).mean().sqrt()).item() for z in ctx["zs"][:-1]]
