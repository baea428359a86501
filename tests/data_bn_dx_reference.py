"""Float64 restatement of the backward apply pass of data_bn (include/sar_hip.h: sar_data_bn_bwd_apply_f32 / _cn8): d loss / d x in
the clip layout (N, C, T, V, M) from dh = d loss / d data_bn(x) in the CN layout [C][N*M*T*V] and the per-channel coefficients
k1..k3 of bn_bwd_finalize (channel ch = v*C + c).

    val  = the value the forward pass normalised: joint, bone (joint minus parent), motion (frame t+1 minus frame t, last frame 0)
           or bone motion -- recomputed from x in FLOAT32 by the forward pass's operations (stream_values)
    dval = k1[ch]*dh + k2[ch]*val + k3[ch]
    motion: df[t] = (t >= 1 ? dval[t-1] : 0) - (t <= T-2 ? dval[t] : 0)              (no motion: df = dval)
    bone:   dx[u] = df[u] - sum over v != u with bone_parent[v] == u of df[v]         (no table: dx = df)
            a self-pair (bone_parent[u] == u: val == 0) forms neither of its two terms, which cancel

Beside dx it returns the MAGNITUDE S of every output element: the sum of |k1*dh| + |k2*val| + |k3| over the dvals that reach it
(a self-pair's none) -- the scale a float32 evaluation's rounding error is bounded against."""
import numpy as np
import torch

HAND_PARENT = np.array([-1, 0, 0, 0, 4], dtype=np.int32)      # V = 5: three children of joint 0, a self-pair, a joint without parent
STREAMS = {"joint": (False, False), "bone": (True, False), "joint_motion": (False, True), "bone_motion": (True, True)}


def ntu_parent():
    from sar_amd.bone import bone_parent_array
    return bone_parent_array()


def stream_values(x, bone_parent, motion):
    """what data_bn normalises, in x's dtype, differentiable: csrc/elementwise.hip load_joint (bone first, then motion)"""
    f = x
    if bone_parent is not None:
        bp = torch.as_tensor(np.asarray(bone_parent), dtype=torch.long)
        has = (bp >= 0).view(1, 1, 1, -1, 1)
        f = torch.where(has, x - x[:, :, :, bp.clamp(min=0), :], x)
    if motion:
        f = torch.cat([f[:, :, 1:] - f[:, :, :-1], torch.zeros_like(f[:, :, :1])], dim=2)
    return f


def cn_to_clip(dh, N, C, T, V, M):
    """CN rows [C][((n*M+m)*T+t)*V+v] -> (N, C, T, V, M)"""
    return dh.reshape(C, N, M, T, V).permute(1, 0, 3, 4, 2)


def clip_to_cn(g):
    N, C, T, V, M = g.shape
    return g.permute(1, 0, 4, 2, 3).reshape(C, N * M * T * V)


def _adjoint(d, bone_parent, motion, sign):
    """the two adjoints on dval (sign = -1) or on the magnitudes (sign = +1: every term counts)"""
    T, V = d.shape[2], d.shape[3]
    if motion:
        df = torch.zeros_like(d)
        if T >= 2:
            df[:, :, 1:] += d[:, :, :T - 1]                       # dval[t-1], t >= 1
            df[:, :, :T - 1] += sign * d[:, :, :T - 1]            # dval[t],   t <= T-2   (dval[T-1] reaches nothing)
    else:
        df = d
    if bone_parent is None:
        return df
    out = torch.zeros_like(df)
    for u in range(V):
        if bone_parent[u] != u:
            out[:, :, :, u] = df[:, :, :, u]
        for v in range(V):
            if bone_parent[v] == u and v != u:
                out[:, :, :, u] += sign * df[:, :, :, v]
    return out


def data_bn_dx(x, dh, k1, k2, k3, bone_parent=None, motion=False):
    """x (N,C,T,V,M) float32; dh [C][N*M*T*V]; k1..k3 [V*C]  ->  (dx, S), both float64 (N,C,T,V,M)"""
    N, C, T, V, M = x.shape
    val = stream_values(x.detach().float(), bone_parent, motion).double()         # float32 operations, as the forward pass
    g = cn_to_clip(dh.detach().double()[:, :N * M * T * V], N, C, T, V, M)
    k = [t.detach().double().reshape(V, C).t().reshape(1, C, 1, V, 1) for t in (k1, k2, k3)]
    dval = k[0] * g + k[1] * val + k[2]
    mag = (k[0] * g).abs() + (k[1] * val).abs() + k[2].abs().expand_as(val)
    return _adjoint(dval, bone_parent, motion, -1.0), _adjoint(mag, bone_parent, motion, 1.0)


def bwd_coefficients(val, dh_clip, gamma, eps):
    """k1..k3 [V*C] by the formulas of bn_bwd_finalize (include/sar_hip.h) from the batch statistics of val (N,C,T,V,M) over (n,m,t)
    and the gradient dh_clip of the normalised tensor in the same layout; float64"""
    N, C, T, V, M = val.shape
    count = N * M * T
    mean = val.mean(dim=(0, 2, 4), keepdim=True)
    var = val.var(dim=(0, 2, 4), unbiased=False, keepdim=True)
    rs = torch.rsqrt(var + eps)
    g = gamma.double().reshape(V, C).t().reshape(1, C, 1, V, 1)
    s1 = dh_clip.sum(dim=(0, 2, 4), keepdim=True)
    dg = rs * (dh_clip * (val - mean)).sum(dim=(0, 2, 4), keepdim=True)
    a, b = s1 / count, dg / count
    flat = lambda t: t.reshape(C, V).t().reshape(V * C)
    return flat(g * rs), flat(-g * rs * rs * b), flat(g * rs * (mean * rs * b - a))
