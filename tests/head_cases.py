"""The shapes and the seeded inputs of tests/test_gpu_head_edges.py, shared with tests/test_head_reference.py so that the CPU file
pins the references, and shows their sensitivity, at exactly what the GPU file launches.  numpy only.  Every shape is there for a
branch of a kernel in csrc/elementwise.hip or csrc/conv2d.hip; DESIGN.md section 4.3 lists which."""
import functools
import zlib

import numpy as np

import head_reference as R

F32, F64 = np.float32, np.float64
TOL = 2e-5          # the per-kernel bar of tests/test_gpu_stgcn_kernels.py (norm-wise: max |a - b| / max |b|)
OPT_TOL = 1e-6      # the optimizer bar of tests/test_gpu_stgcn_kernels.py::test_head_loss_and_sgd (w and v)
BAND = 4.0          # a metric without an earlier bar: within 4x the float32 evaluation's distance from float64


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rel(a, b):
    """max |a - b| / max |b| in float64 (tests/util.py: rel_err)"""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    d = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / (d if d > 0 else 1.0))


def randn(r, *shape):
    return r.standard_normal(shape).astype(F32)


# ---------------------------------------------------------------------------------------------------- pooling
# pool_fwd_kernel: one wave per (sample, channel) over span = Mp TV elements, lane l takes l, l + 64, ..; the 4-way unrolled loop
# runs while i + 192 < span.  span 7: 57 idle lanes; 64 / 75: one trip of the tail loop, some lanes two; 255 / 256 / 257: lanes
# 0..62 / 0..63 / all enter the unrolled loop once (span 257: lane 0 then takes the tail as well); 515: a remainder of 3 behind two trips.
# Mp = 2 doubles every span (14 .. 1030).  Four waves per workgroup: N = 1, 3 leave waves idle, 5 a ragged second workgroup.
POOL_TV = [7, 64, 75, 255, 256, 257, 515]
POOL_N = [1, 3, 4, 5]
POOL_MP = [1, 2]
POOL_C = [3, 20]


def pool_inputs(TV, N, Mp, C):
    r = rng("pool", TV, N, Mp, C)
    return randn(r, C, N * Mp * TV) + F32(0.5), randn(r, N, C)


# ---------------------------------------------------------------------------------------------------- dense layer
# fc_fwd_kernel: C split over 4 waves in chunks of ceil(C / 4), two chains per lane plus an odd tail; K in steps of 64 lanes.
# C = 1, 2, 3: empty waves; 5, 7: a ragged last chunk (2 + 2 + 1 + 0, 2 + 2 + 2 + 1); 257: chunks of 65 (odd) and a last of 62.
# K = 1, 10, 60: idle lanes; 64 / 65: exactly one trip / a second trip with one lane; 120, 129: the class counts and one past 128.
FC_C = [1, 2, 3, 5, 7, 256, 257]
FC_K = [1, 10, 60, 64, 65, 120, 129]
FC_N = [1, 5]
# fc_bwd_w_kernel strides K over 128 threads, fc_bwd_x_kernel C over 256: pairs on both sides of each
FC_BWD = [(1, 1), (3, 129), (7, 120), (5, 65), (256, 60), (257, 129), (257, 1), (256, 128)]


def fc_inputs(C, K, N):
    r = rng("fc", C, K, N)
    return {"feat": randn(r, N, C), "W": randn(r, C, K) * F32(0.1), "bias": randn(r, K) * F32(0.1) + F32(0.3), "dlogits": randn(r, N, K) * F32(0.05)}


# ---------------------------------------------------------------------------------------------------- cross entropy
# softmax_ce_kernel: one workgroup, rows strided over 4 waves, classes over 64 lanes
CE_N = [1, 3, 4, 5, 9]
CE_K = [1, 10, 64, 65, 120, 129]
CE_INV = 1.0 / 16                # the engines pass 1 / global batch, never 1 / N
CE_REGIMES = ["a", "b", "c", "d"]
CE_BAD_K = [10, 65, 129]         # regime (e): a batch of 5 with labels K and -1


def ce_inputs(regime, N, K):
    """(logits float32 (N, K), labels int64 (N)); None where a regime needs two classes and K = 1"""
    r = rng("ce", N, K)
    x, labels = randn(r, N, K), r.integers(0, K, N)
    if regime == "b":                                  # shifted by 1e4 (in float32: the rounded sum is the kernel's input)
        x = x + F32(1e4)
    if regime in ("c", "d") and K == 1:
        return None
    if regime == "c":                                  # one class at 0, every other at -200: exp(-200) underflows in float32
        top = r.integers(0, K, N)
        x = np.full((N, K), -200.0, dtype=F32)
        x[np.arange(N), top] = 0
        labels = (top + 1 + r.integers(0, K - 1, N)) % K
        assert not np.any(labels == top)
    if regime == "d":                                  # one -inf per row, off the label
        off = (labels + 1 + r.integers(0, K - 1, N)) % K
        x[np.arange(N), off] = -np.inf
    return x, labels.astype(np.int64)


def ce_bad_inputs(K):
    """regime (e): (logits, valid labels, the same with row 1 -> K and row 3 -> -1)"""
    x, labels = ce_inputs("a", 5, K)
    bad = labels.copy()
    bad[1], bad[3] = K, -1
    return x, labels, bad


# ---------------------------------------------------------------------------------------------------- optimizers
# both kernels: 256 threads, at most 2048 workgroups, grid stride.  1: one thread; 255 / 257: a ragged workgroup; 2048 * 256 + 257:
# the second trip of the stride loop for 257 threads; 2 * 2048 * 256 + 1: a third trip for one thread.
OPT_N = [1, 255, 257, 2048 * 256 + 257, 2 * 2048 * 256 + 1]
SGD_LR, SGD_MOM = float(F32(0.1)), 0.9           # lr is the float32 value of the device cell
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = float(F32(1e-3)), 0.9, 0.999, 1e-8
STEPS = 3


def nesterov_inputs(n):
    r = rng("sgd", n)
    return randn(r, n), [randn(r, n) for _ in range(STEPS)]


def adam_inputs(n, t0):
    """(w, m, v, [g per step], first step t0 + 1).  Gradient magnitudes span 1e-6 .. 1e3 (n = 1: 1e-6 .. 1e-5, small against
    sqrt(eps), so that the one element can tell where eps stands); element 0 (n > 1) has g = 0 in every step and m = v = 0: its update
    is exactly 0.  w = 0 in both runs, so that the first w IS the update, to float32 precision, and not the update plus the rounding
    of a w of order 1.  t0 = 0: the zero state; t0 = 999: a running state in m and v."""
    r = rng("adam", n, t0)
    hi = 3 if n > 1 else -5
    gs = [(10.0 ** r.uniform(-6, hi, n) * r.choice([-1.0, 1.0], n)).astype(F32) for _ in range(STEPS if t0 == 0 else 1)]
    w, m, v = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    if t0:
        m = (gs[0] * r.uniform(0.2, 1.0, n)).astype(F32)
        v = (gs[0].astype(F64) ** 2 * r.uniform(0.2, 1.0, n)).astype(F32)
    if n > 1:
        for a in gs + [m, v]:
            a[0] = 0
    return w, m, v, gs, t0 + 1


def run_nesterov(n, dt):
    """[(w, v) after each step] in `dt`"""
    w, gs = nesterov_inputs(n)
    v, out = np.zeros(n, F32), []
    for g in gs:
        w, v = R.nesterov_step(w, v, g, SGD_LR, SGD_MOM, dt=dt)
        out.append((w, v))
    return out


def run_adam(n, t0, dt, step=R.adam_step):
    """[(w, m, v) after each step] in `dt`"""
    w, m, v, gs, t = adam_inputs(n, t0)
    out = []
    for i, g in enumerate(gs):
        w, m, v = step(w, m, v, g, t + i, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, dt=dt)
        out.append((w, m, v))
    return out


def updates(w0, ws):
    """w_t - w_{t-1} in float64 of a list of parameter states behind w0"""
    prev, out = np.asarray(w0, dtype=F64), []
    for w in ws:
        out.append(np.asarray(w, dtype=F64) - prev)
        prev = np.asarray(w, dtype=F64)
    return out


# ---------------------------------------------------------------------------------------------------- BatchNorm finalisation
# bn_finalize_kernel / bn_bwd_finalize_kernel: 256 threads per channel, thread i takes parts i, i + 256, ..; four at a time while
# i + 768 < nparts.  1 / 255: the tail loop only, idle threads; 900: threads 0..131 take the unrolled loop, the rest the tail loop;
# 1024: the unrolled loop exactly, no tail; 1029 / 2053: one / two unrolled trips and a tail of 5 threads.
BN_NPARTS = [1, 255, 900, 1024, 1029, 2053]
BN_EPS, BN_MOM = 1e-3, 0.9
BN_CHUNK = 6                     # values per partial: count = 6 nparts
BN_REGIMES = ["unit", "far", "const"]


def _const_partials(nparts):
    """a constant channel whose float32-rounded partials give E x^2 - mean^2 < 0 in exact arithmetic: the first of a fixed list of
    constants that does (most do: each partial carries a rounding of ~6e-8 of 1e6)"""
    for j in range(200):
        c = 1000.0 + 0.37 * (j + 1)
        p = np.stack([np.full(nparts, BN_CHUNK * c), np.full(nparts, BN_CHUNK * c * c)], axis=1).astype(F32)
        s1, s2 = p[:, 0].astype(F64).sum(), p[:, 1].astype(F64).sum()
        count = BN_CHUNK * nparts
        if s2 / count - (s1 / count) ** 2 < -1e-4:
            return p
    raise AssertionError("no constant gives a negative variance")


@functools.lru_cache(maxsize=None)
def bn_partials(regime, nparts):
    """(partials float32 (nparts, 2), count): built in float64 from the values, rounded once"""
    if regime == "const":
        return _const_partials(nparts), BN_CHUNK * nparts
    if regime == "one":                                  # a single value: count = 1, the unbiased switch must not divide by 0
        x = np.array([[3.7]])
    else:
        x = rng("bn", regime, nparts).standard_normal((nparts, BN_CHUNK)) + (1000.0 if regime == "far" else 0.0)
    return np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1).astype(F32), x.size


def bn_case(regimes, nparts):
    """the channels `regimes` side by side: dict(partials (C, nparts, 2), count, gamma, beta, rm, rv)"""
    C = len(regimes)
    parts = [bn_partials(g, nparts) for g in regimes]
    assert len({c for _, c in parts}) == 1
    r = rng("bn affine", regimes, nparts)
    far = np.array([1000.0 if g in ("far", "const") else 0.0 for g in regimes])
    return {"partials": np.stack([p for p, _ in parts]), "count": parts[0][1], "gamma": (1 + 0.1 * randn(r, C)).astype(F32),
            "beta": 0.1 * randn(r, C), "rm": (far * 0.99 + r.standard_normal(C)).astype(F32), "rv": (0.5 + r.random(C)).astype(F32)}


BN_CASES = [(("unit", "far", "const"), n) for n in BN_NPARTS] + [((g,), n) for g in BN_REGIMES for n in BN_NPARTS] + [(("one",), 1)]

# (chan_stride, part_stride, off1, off2) as the engines pass them, for nparts = n: the block tail's four-slot partials read for the
# block's own BatchNorm (slots 0, 1) and for the residual branch's (slots 0, 2), and the two-slot partials of data_bn
BNB_LAYOUTS = [(4, 0, 1), (4, 0, 2), (2, 0, 1)]
BNB_C = 3
BNB_CHUNK = 4


@functools.lru_cache(maxsize=None)
def bnb_case(nparts, centered, dt=F32):
    """x, dz (C, nparts, chunk) float64; mean, rstd, gamma in `dt`; s1, s2 (C, nparts) partials rounded to `dt`; count"""
    r = rng("bnb", nparts)
    x = 0.7 + 1.3 * r.standard_normal((BNB_C, nparts, BNB_CHUNK))
    dz = 0.1 + r.standard_normal((BNB_C, nparts, BNB_CHUNK))
    mean = x.mean(axis=(1, 2)).astype(dt)
    rstd = (1.0 / np.sqrt(x.var(axis=(1, 2)) + BN_EPS)).astype(dt)
    s1 = dz.sum(axis=2).astype(dt)
    s2 = (dz * (x - mean.astype(F64)[:, None, None] if centered else x)).sum(axis=2).astype(dt)
    return {"x": x, "dz": dz, "mean": mean, "rstd": rstd, "gamma": (1 + 0.1 * r.standard_normal(BNB_C)).astype(dt), "s1": s1, "s2": s2,
            "count": nparts * BNB_CHUNK}


def bnb_buffer(case, slots, off1, off2):
    """the (C, nparts, slots) float32 partials buffer: S1 in slot off1, S2 in slot off2, NaN in the slots the call does not name"""
    buf = np.full(case["s1"].shape + (slots,), np.nan, dtype=F32)
    buf[:, :, off1], buf[:, :, off2] = case["s1"], case["s2"]
    return buf


# bn_eval_affine_kernel: one thread per channel, 256 per workgroup; channel 0 has a moving variance of exactly 0
BN_EVAL_C = [1, 64, 256, 257]


def bn_eval_inputs(C):
    r = rng("bn eval", C)
    rv = (0.5 + r.random(C)).astype(F32)
    rv[0] = 0
    return {"gamma": (1 + 0.1 * randn(r, C)).astype(F32), "beta": 0.1 * randn(r, C), "rm": randn(r, C), "rv": rv}


# ---------------------------------------------------------------------------------------------------- re-layouts
# transpose_kernel: 32 x 32 tiles, blockIdx.z = batch.  Ragged tiles in both directions with several batches
TRANSPOSE = [(1, 1, 1), (3, 25, 33), (9, 31, 65), (2, 64, 32), (5, 1, 40)]

# (what, source elements, d0, d1, d2, s0, s1, s2): out[i][j][k] = in[i s0 + j s1 + k s2]
_N, _C, _I, _T, _V, _K, _F, _TAPS, _CIN, _COUT = 3, 5, 7, 4, 6, 3, 4, 9, 5, 7
PERMUTE3 = [
    ("models/gcn.py: (N, C, inner) -> CN", _N * _C * _I, _C, _N, _I, _I, _C * _I, 1),
    ("models/gcn.py: CN -> (N, C, inner)", _N * _C * _I, _N, _C, _I, _I, _N * _I, 1),
    ("models/gcn.py: kernel (C, K F) -> [k][f][c]", _C * _K * _F, _K, _F, _C, _F, 1, _K * _F),
    ("models/stgcn_debug.py: (N, C, T, V) -> [C T][N][V]", _N * _C * _T * _V, _C * _T, _N, _V, _V, _C * _T * _V, 1),
    ("models/stgcn_debug.py: [F T][N][V] -> (N, F, T, V)", _N * _F * _T * _V, _N, _F * _T, _V, _V, _N * _V, 1),
    ("models/stgcn_debug.py: (a, b, inner) -> (b, a, inner)", _N * _C * _I, _C, _N, _I, _I, _C * _I, 1),
    ("conv2d: OIHW -> (tap, c, m)", _COUT * _CIN * _TAPS, _TAPS, _CIN, _COUT, 1, _TAPS, _CIN * _TAPS),
    ("conv2d: OIHW -> (tap, m, c)", _COUT * _CIN * _TAPS, _TAPS, _COUT, _CIN, 1, _CIN * _TAPS, _TAPS),
    ("conv2d: (tap, c, m) gradient -> OIHW", _COUT * _CIN * _TAPS, _COUT, _CIN, _TAPS, 1, _COUT, _CIN * _COUT),
    ("4096 workgroups and a second trip of the stride loop (1 052 929 elements)", 241 * 17 * 257, 17, 241, 257, 257, 17 * 257, 1),
    ("s0 = 0: a broadcast, every source element read four times", 30, 4, 5, 6, 0, 6, 1),
    ("one element", 1, 1, 1, 1, 0, 0, 0),
]

# permute3_batch_kernel: blockIdx.y = item, at most 1024 workgroups of 256 per item, sized by the LARGEST item: for the items of 1
# and 257 elements all but one / two workgroups must do nothing; the large one takes a second trip of the stride loop for 3 threads.
# (src_off, dst_off, d0, d1, d2, s0, s1, s2); the destinations, in launch order: [1, 262148), [262153, 262410), [0, 1): the first
# two ranges adjacent to each other in memory order (0 | 1 ..), a gap of 5 behind the large one, offsets not monotonic
PB_BIG = 1024 * 256 + 3
PB_ITEMS = [(300, 1, PB_BIG, 1, 1, 2, 0, 0),                 # every second source element
            (40 + 256, PB_BIG + 6, 1, 257, 1, 0, -1, 0),     # source elements 296 down to 40: a negative stride
            (7, 0, 1, 1, 1, 0, 0, 0)]
PB_SRC = 300 + 2 * PB_BIG
PB_DST = PB_BIG + 6 + 257


def permute_batch_expected(src, fill):
    """the destination buffer of PB_DST elements that started as `fill`"""
    out = np.full(PB_DST, fill, dtype=F32)
    for so, do, d0, d1, d2, s0, s1, s2 in PB_ITEMS:
        out[do:do + d0 * d1 * d2] = R.permute3(src, d0, d1, d2, s0, s1, s2, src_off=so)
    return out


# ---------------------------------------------------------------------------------------------------- the measured yardsticks
ADAM_METRICS = {"adam update, step 1": (0, [0]), "adam update, steps 2 and 3": (0, [1, 2]), "adam update, step 1000": (999, [0])}


def adam_metric(t0, i):
    """the yardstick of step i of the run that starts behind step t0"""
    return next(k for k, (t, steps) in ADAM_METRICS.items() if t == t0 and i in steps)



@functools.lru_cache(maxsize=None)
def float32_distance(metric):
    """the worst distance, over the cases of `metric`, of head_reference evaluated in float32 from its float64 evaluation: X of
    "kernel within 4 X".  The worst over the cases and not each case's own figure: one case's float32 evaluation is a single draw of
    its roundings and can land arbitrarily close."""
    worst = 0.0
    if metric in ADAM_METRICS:
        t0, steps = ADAM_METRICS[metric]
        for n in OPT_N:
            w0 = adam_inputs(n, t0)[0]
            u32, u64 = updates(w0, [s[0] for s in run_adam(n, t0, F32)]), updates(w0, [s[0] for s in run_adam(n, t0, F64)])
            worst = max([worst] + [rel(u32[i], u64[i]) for i in steps])
    elif metric == "nesterov update":
        for n in OPT_N:
            w0 = nesterov_inputs(n)[0]
            u32, u64 = updates(w0, [s[0] for s in run_nesterov(n, F32)]), updates(w0, [s[0] for s in run_nesterov(n, F64)])
            worst = max([worst] + [rel(a, b) for a, b in zip(u32, u64)])
    elif metric in ("shifted probs", "shifted dlogits", "shifted loss"):
        # regime (b): the float32 evaluation of the shifted logits against the float64 evaluation of the UNSHIFTED ones (probs,
        # dlogits) -- the rounding of x + 1e4 to float32 is part of the figure -- and of the shifted ones (loss)
        for N in CE_N:
            for K in CE_K:
                (xa, lab), (xb, _) = ce_inputs("a", N, K), ce_inputs("b", N, K)
                l32, d32, p32 = R.softmax_ce(xb, lab, CE_INV, dt=F32)
                _, da, pa = R.softmax_ce(xa, lab, CE_INV)
                lb = R.softmax_ce(xb, lab, CE_INV)[0]
                worst = max(worst, {"shifted probs": rel(p32, pa), "shifted dlogits": rel(d32, da), "shifted loss": rel(l32, lb)}[metric])
    elif metric == "far channel":                      # rstd of the mean-1000 channel alone, from the same float32 partials (a record:
                                                       # 4 X is no bar there, the channel is held to TOL)
        for n in BN_NPARTS:
            c = bn_case(("far",), n)
            worst = max(worst, rel(R.bn_finalize(c["partials"], c["count"], BN_EPS, BN_MOM, 1, dt=F32)["rstd"],
                                   R.bn_finalize(c["partials"], c["count"], BN_EPS, BN_MOM, 1)["rstd"]))
    else:
        raise KeyError(metric)
    return worst
