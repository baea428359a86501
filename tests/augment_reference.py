"""numpy restatement of the augmentation contract (DESIGN.md "Augmentation"; csrc/augment.hip implements the same six items).

    augment(x, table, crop, mode="float64")   x (N, 3, T, V, M) float32, table (N, 16) float32 -> (N, 3, T, V, M) in `mode`

mode "float64": the blend, the matrix product, the scale and the shift in float64 from the float32 clip, the float32 blend weight w
and the float32-rounded matrix entries (both are part of the contract); s(tau) and d(tau) stay double.
mode "float32": the same formulas with every per-coordinate operation in float32 (s, d rounded to float32 first), one rounding per
operation, no fused multiply-add: what a plain fp32 implementation computes, and the yardstick for the kernel's distance from the
float64 result.  p L, o (L - Lc + 1), the time map, tau, the parameter interpolation and the trigonometry are double in both."""
import numpy as np


def valid_length(clip):
    """one past the last frame of (3, T, V, M) with a non-zero coordinate"""
    nz = np.nonzero((clip != 0).any(axis=(0, 2, 3)))[0]
    return int(nz[-1]) + 1 if nz.size else 0


def time_map(L, p, o, T):
    """(b, Lc, i0[T], i1[T], frac[T] in double) of items 2 and 3; p, o are the float32 table values"""
    p, o = float(np.float32(p)), float(np.float32(o))
    Lc = min(max(1, int(np.floor(p * L))), L)              # (p <= 1 in every drawn table; the kernel clamps the same way)
    b = max(min(int(np.floor(o * (L - Lc + 1))), L - Lc), 0)
    t = np.arange(T, dtype=np.float64)
    s = np.clip((t + 0.5) * Lc / T - 0.5, 0.0, float(Lc - 1))
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, Lc - 1)
    return b, Lc, i0, i1, s - i0


def rotation(alpha, beta, gamma):
    """R = Rz(gamma) Ry(beta) Rx(alpha), (..., 3, 3) in double"""
    a, b, g = (np.asarray(v, dtype=np.float64) for v in (alpha, beta, gamma))
    sa, ca, sb, cb, sg, cg = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(g), np.cos(g)
    R = np.empty(a.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cb * cg, sa * sb * cg - ca * sg, ca * sb * cg + sa * sg
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = cb * sg, sa * sb * sg + ca * cg, ca * sb * sg - sa * cg
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sb, sa * cb, ca * cb
    return R


def frame_parameters(row, T):
    """(R (T, 3, 3) float32, s (T,) double, d (T, 3) double) of item 5 from one float32 table row"""
    row = np.asarray(row, dtype=np.float32).astype(np.float64)
    tau = np.arange(T, dtype=np.float64) / (T - 1) if T > 1 else np.zeros(1)
    q = row[None, 2:9] + tau[:, None] * (row[None, 9:16] - row[None, 2:9])
    return rotation(q[:, 0], q[:, 1], q[:, 2]).astype(np.float32), q[:, 3], q[:, 4:7]


def augment_clip(clip, row, crop, mode="float64", exact_weights=False, terms=None):
    """one clip (3, T, V, M) float32.  exact_weights keeps the blend weight in double (only for the comparison of the time map with
    torch's interpolate).  terms: a dict that receives 'norm' (T, V, M) = max(|near joint|, |far joint|) in double."""
    dt = np.float64 if mode == "float64" else np.float32
    clip = np.asarray(clip, dtype=np.float32)
    _, T, V, M = clip.shape
    L, p, o = (valid_length(clip), row[0], row[1]) if crop else (T, 1.0, 0.0)
    if terms is not None:
        terms["norm"] = np.zeros((T, V, M))
    if L == 0:
        return np.zeros(clip.shape, dtype=dt)
    b, Lc, i0, i1, frac = time_map(L, p, o, T)
    assert 0 <= b and b + Lc <= L
    x0, x1 = clip[:, b + i0].astype(dt), clip[:, b + i1].astype(dt)
    n0, n1 = (x0 == 0).all(axis=0), (x1 == 0).all(axis=0)                      # (T, V, M)
    near1 = (frac > 0.5)[:, None, None]                                        # i0 wins a tie
    near, near_null, far_null = np.where(near1, x1, x0), np.where(near1, n1, n0), np.where(near1, n0, n1)
    assert not exact_weights or dt is np.float64
    w = (frac if exact_weights else frac.astype(np.float32)).astype(dt)[None, :, None, None]
    u = np.where(far_null, near, (dt(1) - w) * x0 + w * x1)
    R, s, d = frame_parameters(row, T)
    R, s, d = R.astype(u.dtype), s.astype(u.dtype), d.astype(u.dtype)
    out = np.empty_like(u)
    for i in range(3):
        acc = R[:, i, 0, None, None] * u[0] + R[:, i, 1, None, None] * u[1]
        acc = acc + R[:, i, 2, None, None] * u[2]
        out[i] = s[:, None, None] * acc + d[:, i, None, None]
    out[:, near_null] = 0
    if terms is not None:
        terms["norm"] = np.maximum(np.sqrt((x0.astype(np.float64) ** 2).sum(0)), np.sqrt((x1.astype(np.float64) ** 2).sum(0)))
    return out


def augment(x, table, crop=False, mode="float64", terms=None):
    """the batch; terms: a list that receives one dict per clip (see augment_clip)"""
    x, table = np.asarray(x), np.asarray(table, dtype=np.float32)
    assert x.dtype == np.float32 and x.ndim == 5 and x.shape[1] == 3 and table.shape == (x.shape[0], 16)
    outs = []
    for n in range(x.shape[0]):
        tm = {} if terms is not None else None
        outs.append(augment_clip(x[n], table[n], crop, mode, terms=tm))
        if terms is not None:
            terms.append(tm)
    return np.stack(outs) if outs else np.zeros(x.shape, dtype=np.float64 if mode == "float64" else np.float32)


def bound(x, table, crop=False):
    """(ref64, bar): the float64 result and, per output coordinate, 8 * 2^-24 * (max(|near joint|, |far joint|) * s_max + d_max)
    with s_max, d_max the larger of the two key frames' scale and |shift component| of the clip"""
    terms = []
    ref = augment(x, table, crop, "float64", terms=terms)
    table = np.asarray(table, dtype=np.float32).astype(np.float64)
    bar = np.empty(ref.shape)
    for n, tm in enumerate(terms):
        s_max = max(abs(table[n, 5]), abs(table[n, 12]))
        d_max = max(np.abs(table[n, 6:9]).max(), np.abs(table[n, 13:16]).max())
        bar[n] = 8.0 * 2.0 ** -24 * (tm["norm"][None] * s_max + d_max)
    return ref, bar
