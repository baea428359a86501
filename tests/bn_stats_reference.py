"""BatchNorm batch statistics at a LOCATION: float64 definitions, seeded channels at a requested mean/std, and float32 restatements
of the summation structure of the kernels that produce the (sum, sum of squares) partials (include/sar_hip.h, "Batch-norm plumbing").

Definitions (float64, over the samples of one channel):
    mean = sum x / n ; var = sum (x - mean)^2 / n (biased) ; rstd = 1 / sqrt(var + eps)
    scale = gamma * rstd ; shift = beta - mean * scale ; y = x * scale + shift
    moving_mean = momentum * moving_mean + (1 - momentum) * mean ; moving_var likewise with var (data_bn: biased) or
    var * n / (n - 1) (the blocks: unbiased)

Restatements (numpy float32 inside one partial, float64 across partials, as sar_bn_finalize_f32 reduces them):
    data_bn, csrc/elementwise.hip data_bn_reduce_kernel: one workgroup per (clip n, coordinate c); thread (row group rg, joint v,
    body m) chains s1 += x, s2 = fma(x, x, s2) over t = rg, rg + groups, .. with groups = 256 // (V*M); joint v then adds its
    groups * M thread sums in float32, g outer and m inner: ONE partial per clip and channel, float64 over the N clips.
      one pass:  the sums of x and x^2, var = S2/n - mean^2                                         (sar_data_bn_stats_f32)
      two pass:  pivot p = float32(mean of the first pass) where that mean lies more than 2 first-pass standard deviations
                 from 0, else p = 0 (the first-pass sums stand); the sums of (x - p) and (x - p)^2,
                 mean = p + S1/n, var = S2/n - (S1/n)^2                                             (sar_data_bn_stats_pivot_f32)
    apply: y = fma(x, scale, shift) in float32 with scale and shift rounded to float32 (data_bn_apply_kernel); apply_no_fma rounds
    the product first.

The error of a channel is max |y - y64| / max |y64| with y64 the float64 normalised output of the SAME float32 samples."""
import numpy as np

EPS = 1e-3
TPB = 256
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------- float64 definitions
def stats64(x, eps=EPS, gamma=1.0, beta=0.0):
    """x (..., samples) -> dict of float64 arrays (...): mean, var (biased), rstd, scale, shift"""
    x = np.asarray(x, f64)
    mean = x.mean(axis=-1)
    var = ((x - mean[..., None]) ** 2).mean(axis=-1)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)


def normalised64(x, st):
    return np.asarray(x, f64) * st["scale"][..., None] + st["shift"][..., None]


def moving_update64(moving_mean, moving_var, mean, var, count, momentum, unbiased):
    vr = var * count / (count - 1.0) if (unbiased and count > 1) else var
    return momentum * moving_mean + (1.0 - momentum) * mean, momentum * moving_var + (1.0 - momentum) * vr


def channel_error(y, y64):
    """max |y - y64| / max |y64| over the last axis"""
    y, y64 = np.asarray(y, f64), np.asarray(y64, f64)
    return np.abs(y - y64).max(axis=-1) / np.abs(y64).max(axis=-1)


# ---------------------------------------------------------------------------------------------- seeded channels
def _zscore(z):
    z = np.asarray(z, f64)
    ax = tuple(range(1, z.ndim))
    z = z - z.mean(axis=ax, keepdims=True)
    return z / np.sqrt((z ** 2).mean(axis=ax, keepdims=True))


def white(seed, draws, N, T, M, ratio):
    """(draws, N, T, M) float32: white noise, z-scored per draw in float64, then the offset `ratio` (std = 1)"""
    rng = np.random.default_rng([seed, 1])
    return (_zscore(rng.standard_normal((draws, N, T, M))) + ratio).astype(f32)


def trajectory(seed, draws, N, T, M, ratio):
    """a per-clip offset plus a random walk over t, z-scored per draw in float64, then the offset"""
    rng = np.random.default_rng([seed, 2])
    z = rng.standard_normal((draws, N, 1, M)) * 3.0 + np.cumsum(rng.standard_normal((draws, N, T, M)), axis=2) * 0.3
    return (_zscore(z) + ratio).astype(f32)


def constant(draws, N, T, M, value):
    return np.full((draws, N, T, M), value, f32)


def zero(draws, N, T, M):
    return np.zeros((draws, N, T, M), f32)


def second_body_zero(seed, draws, N, T, M, ratio):
    """the first body a white channel at `ratio`, every other body exactly 0 in every clip (M >= 2)"""
    assert M >= 2
    out = np.zeros((draws, N, T, M), f32)
    out[..., :1] = white(seed + 77, draws, N, T, 1, ratio)
    return out


# ---------------------------------------------------------------------------------------------- float32 restatements
def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32 (a double
    rounding differs from the single one in about 2^-29 of the cases, by one float32 ulp)"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def data_bn_partials(x, V=25, pivot=None):
    """x (..., N, T, M) float32, the samples of ONE joint's channel -> partials (..., N, 2) float32 of the workgroup of each clip.
    pivot (...) float32 or None: subtracted from every sample first (one float32 rounding, as the kernel)"""
    x = np.asarray(x, f32)
    N, T, M = x.shape[-3:]
    assert V * M <= TPB
    groups = TPB // (V * M)
    if pivot is not None:
        x = (x - np.asarray(pivot, f32)[..., None, None, None]).astype(f32)
    lead = x.shape[:-2]
    s1 = np.zeros(lead + (groups, M), f32)
    s2 = np.zeros(lead + (groups, M), f32)
    for t0 in range(0, T, groups):                      # thread (rg, m): t = rg, rg + groups, ..
        v = x[..., t0:t0 + groups, :]
        k = v.shape[-2]
        s1[..., :k, :] = s1[..., :k, :] + v
        s2[..., :k, :] = _fma32(v, v, s2[..., :k, :])
    a = np.zeros(lead, f32)
    b = np.zeros(lead, f32)
    for g in range(groups):                             # joint v's thread: g outer, m inner
        for m in range(M):
            a = (a + s1[..., g, m]).astype(f32)
            b = (b + s2[..., g, m]).astype(f32)
    return np.stack([a, b], axis=-1)


def block_partials(u, length):
    """u (..., columns) float32 -> partials (..., ceil(columns / length), 2): a float32 chain (s1 += u, s2 = fma(u, u, s2)) inside
    each run of `length` columns -- the structure of a GEMM epilogue that leaves one partial per output row and column block"""
    u = np.asarray(u, f32)
    n = u.shape[-1]
    nparts = -(-n // length)
    pad = np.zeros(u.shape[:-1] + (nparts * length - n,), f32)
    w = np.concatenate([u, pad], axis=-1).reshape(u.shape[:-1] + (nparts, length))
    s1 = np.zeros(w.shape[:-1], f32)
    s2 = np.zeros(w.shape[:-1], f32)
    for i in range(length):
        s1 = (s1 + w[..., i]).astype(f32)
        s2 = _fma32(w[..., i], w[..., i], s2)
    return np.stack([s1, s2], axis=-1)


def finalize(partials, count, eps=EPS, gamma=1.0, beta=0.0, pivot=None):
    """bn_finalize_kernel: partials (..., nparts, 2) float32 summed in float64; outputs rounded to float32 as the kernel stores them"""
    p = np.asarray(partials, f64)
    m1 = p[..., 0].sum(axis=-1) / count
    var = np.maximum(p[..., 1].sum(axis=-1) / count - m1 * m1, 0.0)
    mean = m1 if pivot is None else np.asarray(pivot, f64) + m1
    rstd = 1.0 / np.sqrt(var + eps)
    return dict(mean=mean, var=var, rstd=rstd, scale=(gamma * rstd).astype(f32), shift=(beta - mean * gamma * rstd).astype(f32),
                scale64=gamma * rstd, shift64=beta - mean * gamma * rstd)


PIVOT_RATIO = 2.0


def pivot_of(partials, count):
    """bn_pivot_kernel: the float32 mean of the first pass where mean^2 > PIVOT_RATIO^2 var by the first pass's own statistics
    (var <= 0 beside a mean that is not 0 included), else 0: such a channel keeps its first-pass sums"""
    p = np.asarray(partials, f64)
    m = p[..., 0].sum(axis=-1) / count
    var = p[..., 1].sum(axis=-1) / count - m * m
    return np.where(m * m > PIVOT_RATIO ** 2 * var, m, 0.0).astype(f32)


def data_bn_one_pass(x, V=25, **kw):
    N, T, M = x.shape[-3:]
    return finalize(data_bn_partials(x, V), N * T * M, **kw)


def data_bn_two_pass(x, V=25, **kw):
    N, T, M = x.shape[-3:]
    p = pivot_of(data_bn_partials(x, V), N * T * M)
    return finalize(data_bn_partials(x, V, pivot=p), N * T * M, pivot=p, **kw)


def block_stats(u, length, **kw):
    return finalize(block_partials(u, length), u.shape[-1], **kw)


def apply_fma(x, scale, shift):
    x = np.asarray(x, f32)
    e = (Ellipsis,) + (None,) * (x.ndim - np.ndim(scale))
    return _fma32(x, np.asarray(scale, f32)[e], np.asarray(shift, f32)[e])


def apply_no_fma(x, scale, shift):
    x = np.asarray(x, f32)
    e = (Ellipsis,) + (None,) * (x.ndim - np.ndim(scale))
    return ((x * np.asarray(scale, f32)[e]).astype(f32) + np.asarray(shift, f32)[e]).astype(f32)


# ---------------------------------------------------------------------------------------------- errors of a restatement
def stats_only_error(x, st):
    """worst channel error of (x - mean) * rstd formed in float64 from a restatement's statistics: (draws, N, T, M) -> float"""
    flat = np.asarray(x, f64).reshape(x.shape[0], -1)
    y = (flat - st["mean"][:, None]) * st["rstd"][:, None]
    return float(channel_error(y, normalised64(flat, stats64(flat))).max())


def applied_error(x, st, apply=apply_fma):
    """worst channel error of the float32 output y = apply(x, scale, shift) of a restatement"""
    flat = np.asarray(x, f32).reshape(x.shape[0], -1)
    return float(channel_error(apply(flat, st["scale"], st["shift"]), normalised64(flat, stats64(flat))).max())


def exact_stats_f32(x):
    """float64 statistics with scale and shift rounded to float32: what the apply pass alone is given"""
    flat = np.asarray(x, f64).reshape(x.shape[0], -1)
    st = stats64(flat)
    return dict(st, scale=st["scale"].astype(f32), shift=st["shift"].astype(f32))


# The envelope tests/test_gpu_bn_stats_location.py asserts; tests/test_bn_stats_reference.py validates every (restatement, ratio, bar)
# of it on the CPU (worst error of 100 seeded draws <= bar / 2).
BAR = 2e-5
DATA_BN_RATIOS = (0, 8, 64)         # asserted at BAR
DATA_BN_RECORDED = 256              # asserted at 4 x the two-pass-plus-apply restatement, value recorded

# The convolution epilogues (SAR_EPI_STATS: one partial per output row and column block, csrc/conv_epi_f32.h) at the GPU test's
# shapes leave partials of 52 to 57 columns (sar_conv_gemm_nparts).  The one-pass sums of such a partial, restated as ONE float32
# chain, hold half the bar up to mean/std 8; at 16 the chain leaves 1.1e-5 to 1.2e-5, more than half of 2e-5, so 16 is lowered to 8
# for these producers and 16 joins 64 among the recorded ratios.  (The kernels add 4 values per lane and then a 16-wide and a 2-wide
# tree, which rounds less than a chain: the restatement is the pessimistic one.)
CONV_RATIOS = (0, 4, 8)
CONV_RECORDED = (16, 64)
CONV_COLUMNS = 2050
# The same ratios hold for every partial of at most 64 columns (a chain of 64 leaves 4.0e-6 at 8 and 1.6e-5 at 16): the CN8 epilogues
# and sar_conv2d_gemm_f32 / _split (50 columns for the 3x3 layer at (16, 32, 20 x 20, B = 4), 64 for the 7x7 stem at B = 2, 25 split).
CONV_MAX_LENGTH = 64
# sar_gin_sum_fwd_f32 at 2 050 columns: 9 partials of 228.  The chain holds half the bar at 4 (3.2e-6) and not at 8 (1.3e-5); the sum
# of rectified branches is never centred, so the smallest ratio asserted is 1.
GIN_RATIOS = (1, 4)
GIN_MAX_LENGTH = 228

# The dense-adjacency contractions (sar_graph_dense_fwd_f32: 187 columns per partial at 82 frames; sar_graph_dense_t_fwd_f32: 94).
# The chain of 187 leaves 1.06e-5 at mean/std 8, so the first asserts 0 and 4 only; the chain of 94 holds 8 (6.7e-6).
DENSE_RATIOS = (0, 4)
DENSE_T_RATIOS = (0, 4, 8)
DENSE_FRAMES = 82
