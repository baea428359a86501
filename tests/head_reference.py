"""What the kernels that end every training step compute, restated in numpy: the head (pooling, dense layer, cross entropy), the two
optimizers, the BatchNorm finalisations and the weight re-layouts (csrc/elementwise.hip, csrc/conv2d.hip; include/sar_hip.h states
each contract).  No torch, no GPU.  tests/test_head_reference.py pins every function to torch float64 autograd and to the oracles;
tests/test_gpu_head_edges.py holds the kernels to them.

Every function takes `dt`: float64 is the reference; float32 evaluates the same formulas with float32 inputs, constants and
arithmetic (numpy rounds every operation of a float32 array to float32) -- the yardstick for a metric no earlier test has a bar
for: the kernel must be within 4x the float32 evaluation's distance from the float64 one."""
import numpy as np

F64 = np.float64


def _a(x, dt):
    return np.asarray(x).astype(dt)


# ---------------------------------------------------------------------------------------------------- head
def pool_fwd(y, N, Mp, TV, dt=F64):
    """y CN [C][N Mp TV] -> feat [N][C]: the mean over the TV positions of a sequence, then over the Mp persons of a sample"""
    y = _a(y, dt)
    C = y.shape[0]
    return y.reshape(C, N, Mp, TV).mean(axis=3, dtype=dt).mean(axis=2, dtype=dt).T.copy()


def pool_bwd(dfeat, N, Mp, TV, dt=F64):
    """dfeat [N][C] -> dy [C][N Mp TV]: every position of sample n receives dfeat[n][c] / (Mp TV)"""
    d = _a(dfeat, dt).T / dt(Mp * TV)
    return np.repeat(d[:, :, None], Mp * TV, axis=2).reshape(d.shape[0], N * Mp * TV)


def fc_fwd(feat, W, bias, dt=F64):
    out = _a(feat, dt) @ _a(W, dt)
    return out if bias is None else out + _a(bias, dt)


def fc_bwd(feat, W, dlogits, dt=F64):
    """(dW [C][K], dbias [K], dfeat [N][C])"""
    feat, W, dl = _a(feat, dt), _a(W, dt), _a(dlogits, dt)
    return feat.T @ dl, dl.sum(axis=0, dtype=dt), dl @ W.T


def softmax_ce(logits, labels, inv_global_batch, dt=F64):
    """(loss_sum, dlogits, probs): loss_i = logsumexp(row i) - row i[label i]; loss_sum = inv_global_batch * sum_i loss_i;
    dlogits = (probs - onehot) * inv_global_batch.  A label outside [0, K) has no class: the loss is NaN and that row's dlogits
    are NaN; probs do not depend on the labels."""
    x = _a(logits, dt)
    N, K = x.shape
    labels = np.asarray(labels).astype(np.int64)
    inv = dt(inv_global_batch)
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx)
    se = e.sum(axis=1, keepdims=True, dtype=dt)
    probs = e / se
    lse = np.log(se[:, 0]) + mx[:, 0]
    ok = (labels >= 0) & (labels < K)
    lab = np.where(ok, labels, 0)
    loss = np.where(ok, lse - x[np.arange(N), lab], dt(np.nan))
    onehot = np.zeros((N, K), dtype=dt)
    onehot[np.arange(N), lab] = 1
    dlogits = (probs - onehot) * inv
    dlogits[~ok] = np.nan
    return loss.sum(dtype=dt) * inv, dlogits, probs


# ---------------------------------------------------------------------------------------------------- optimizers
def nesterov_step(w, v, g, lr, momentum=0.9, dt=F64):
    """oracle.stgcn.sgd_nesterov_step: v <- momentum v - lr g; w <- w + (momentum v - lr g).  Returns (w, v)."""
    w, v, g = _a(w, dt), _a(v, dt), _a(g, dt)
    v = v * dt(momentum) - dt(lr) * g
    return w + (dt(momentum) * v - dt(lr) * g), v


def adam_step(w, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8, dt=F64):
    """oracle.resnet.adam_step at step t >= 1 (torch.optim.Adam's defaults).  The betas are Python doubles and b ** t is formed in
    double in every `dt`: the float32 evaluation rounds b ** t and forms 1 - b ** t in float32.  Returns (w, m, v)."""
    w, m, v, g = _a(w, dt), _a(m, dt), _a(v, dt), _a(g, dt)
    m = m * dt(b1) + dt(1 - b1) * g
    v = v * dt(b2) + dt(1 - b2) * g * g
    bc1, bc2 = dt(1) - dt(b1 ** t), dt(1) - dt(b2 ** t)
    denom = np.sqrt(v) / np.sqrt(bc2) + dt(eps)
    return w + (-dt(lr) / bc1) * (m / denom), m, v


# ---------------------------------------------------------------------------------------------------- BatchNorm
def bn_finalize(partials, count, eps, momentum, unbiased_running, gamma=None, beta=None, running_mean=None, running_var=None, dt=F64):
    """partials [C][nparts][2] = (sum x, sum x^2) over `count` values per channel.  mean; var = E x^2 - mean^2, biased, never below 0
    (rounded partials of a constant channel can give less); rstd = 1 / sqrt(var + eps); scale = gamma rstd; shift = beta - mean scale;
    moving <- momentum moving + (1 - momentum) batch, the variance as var count / (count - 1) when unbiased_running and count > 1.
    Returns a dict; the moving statistics only when given."""
    p = _a(partials, dt)
    C = p.shape[0]
    count = dt(count)
    s1, s2 = p[:, :, 0].sum(axis=1, dtype=dt), p[:, :, 1].sum(axis=1, dtype=dt)
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, dt(0))
    rstd = dt(1) / np.sqrt(var + dt(eps))
    g = np.ones(C, dtype=dt) if gamma is None else _a(gamma, dt)
    b = np.zeros(C, dtype=dt) if beta is None else _a(beta, dt)
    out = {"mean": mean, "var": var, "rstd": rstd, "scale": g * rstd, "shift": b - mean * (g * rstd)}
    if running_mean is not None:
        vr = var * count / (count - dt(1)) if (unbiased_running and count > 1) else var
        out["running_mean"] = dt(momentum) * _a(running_mean, dt) + (dt(1) - dt(momentum)) * mean
        out["running_var"] = dt(momentum) * _a(running_var, dt) + (dt(1) - dt(momentum)) * vr
    return out


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, dt=F64):
    """(scale, shift) of inference: y = gamma (x - moving mean) / sqrt(moving var + eps) + beta"""
    rm, rv = _a(running_mean, dt), _a(running_var, dt)
    rstd = dt(1) / np.sqrt(rv + dt(eps))
    g = np.ones_like(rm) if gamma is None else _a(gamma, dt)
    b = np.zeros_like(rm) if beta is None else _a(beta, dt)
    return g * rstd, b - rm * g * rstd


def bn_bwd_finalize(s1_parts, s2_parts, centered, count, gamma, mean, rstd, dt=F64):
    """From the BatchNorm backward formula.  y = gamma xhat + beta with xhat = (x - mean) rstd over `count` values per channel:
        dbeta = sum dz,   dgamma = sum dz xhat,   dx = gamma rstd (dz - dbeta / count - xhat dgamma / count).
    The partials [C][nparts] hold S1 = sum dz and S2 = sum dz (x - mean) when `centered`, else sum dz x, so
    dgamma = rstd S2 (centered) or rstd (S2 - mean S1).  dx is affine in (dz, x): dx = k1 dz + k2 x + k3; collecting terms,
        k1 = gamma rstd,   k2 = -gamma rstd^2 dgamma / count,   k3 = gamma rstd (mean rstd dgamma - dbeta) / count.
    Returns dict(dgamma, dbeta, k1, k2, k3)."""
    S1, S2 = _a(s1_parts, dt).sum(axis=1, dtype=dt), _a(s2_parts, dt).sum(axis=1, dtype=dt)
    mean, rstd, count = _a(mean, dt), _a(rstd, dt), dt(count)
    g = np.ones_like(mean) if gamma is None else _a(gamma, dt)
    dgamma = rstd * S2 if centered else rstd * (S2 - mean * S1)
    return {"dgamma": dgamma, "dbeta": S1, "k1": g * rstd, "k2": -g * rstd * rstd * dgamma / count,
            "k3": g * rstd * (mean * rstd * dgamma - S1) / count}


# ---------------------------------------------------------------------------------------------------- re-layouts
def transpose(x, batch, R, Cc):
    """[batch][R][Cc] -> [batch][Cc][R], flat"""
    return np.ascontiguousarray(np.asarray(x).reshape(batch, R, Cc).transpose(0, 2, 1)).reshape(-1)


def permute3(src, d0, d1, d2, s0, s1, s2, src_off=0):
    """out[i][j][k] (contiguous, flat) = src[src_off + i s0 + j s1 + k s2]; a stride may be 0 (a broadcast) or negative"""
    i, j, k = np.arange(d0, dtype=np.int64), np.arange(d1, dtype=np.int64), np.arange(d2, dtype=np.int64)
    idx = src_off + i[:, None, None] * s0 + j[None, :, None] * s1 + k[None, None, :] * s2
    assert idx.min() >= 0 and idx.max() < np.asarray(src).size, "permute3: the index map leaves the source"
    return np.asarray(src).reshape(-1)[idx].reshape(-1)
