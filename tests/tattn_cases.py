"""The shared cases of the TemporalAttention tests: (N, C, T, V, num_hidden, seed).  The seed is part of the case: it is chosen so that
every hidden pre-activation of the float64 run is at least 1e-5 of its layer's RMS away from zero (tests/test_tattn_reference.py
asserts it), which keeps ReLU flips between float32 and float64 out of the compared gradients."""
import functools
import math

import torch

import tattn_reference as R

LISTED = [
    (3, 5, 7, 25, (6,), 0),             # nothing a multiple of anything
    (2, 64, 33, 25, (64,), 0),
    (2, 256, 9, 25, (128, 64), 0),      # K = 6 400, the widest layer
    (2, 7, 40, 11, (), 0),              # no hidden layer, sigmoid in the first product
    (1, 64, 130, 25, (33, 5), 0),       # rows just over a 128 tile, odd widths
    (2, 16, 300, 25, (128,), 17),       # full clip length; the first weight gradient in 5 slabs
    (1, 3, 1, 25, (4,), 0),             # one frame
    (2, 8, 5, 1, (3,), 0),              # V = 1
]
# sizes at which csrc/tattn.hip takes another path
EDGES = [
    (3, 6, 70, 40, (20, 3), 1),         # V > 32: two K steps per channel in the score (32 + 8 joints), two joint blocks in wgrad / dx
    (1, 4, 9, 64, (40,), 0),            # V = 64, the limit: full K steps, no spare lane in the walks
    (2, 3, 35, 33, (7,), 0),            # V = 33: a K step of one joint (padded to two); frames 32 .. 34 in a tile of their own
    (5, 9, 13, 25, (97,), 0),           # rows 65 = one over the score tile; units over 96: all four unit blocks; C = 9 = 2 groups + 1
    (1, 4, 64, 25, (32,), 0),           # rows = exactly one score tile, frames = exactly two wgrad tiles, one unit block
]
CASES = LISTED + EDGES
SMALL = [LISTED[0], LISTED[3], EDGES[2]]      # the guard-band cases


def case_id(case):
    N, C, T, V, hidden, seed = case
    return "%dx%dx%dx%d-%s" % (N, C, T, V, "_".join(map(str, hidden)) or "none")


def make_params(C, V, hidden, gen):
    """glorot-uniform kernels, biases 0.1 randn (float64)"""
    params, fan_in = [], V * C
    for units in list(hidden) + [1]:
        limit = math.sqrt(6.0 / (fan_in + units))
        params.append((torch.rand(fan_in, units, generator=gen, dtype=torch.float64) * 2 - 1) * limit)
        params.append(0.1 * torch.randn(units, generator=gen, dtype=torch.float64))
        fan_in = units
    return params


def make_case(case):
    """(x, dout, params) in float64"""
    N, C, T, V, hidden, seed = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, T, V, generator=gen, dtype=torch.float64)
    dout = torch.randn(N, C, T, V, generator=gen, dtype=torch.float64)
    return x, dout, make_params(C, V, hidden, gen)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, float64 run, float32 run), computed once and shared, never modified; a run = dict of out, a (N T), dx, grads, and the
    intermediates h1 (units_1, N T), dz1 (units_1, N T), dzL (N T), margins (float64 only)"""
    x, dout, params = make_case(case)
    runs = []
    for dt in (torch.float64, torch.float32):
        out, ctx = R.forward(x.to(dt), [p.to(dt) for p in params])
        dx, grads, dzs = R.backward(ctx, dout.to(dt))
        runs.append(dict(out=out, a=ctx["a"].reshape(-1), dx=dx, grads=grads, h1=ctx["hs"][1].t().contiguous(), dz1=dzs[0].t().contiguous(),
                         dzL=dzs[-1].reshape(-1), margins=R.relu_margins(ctx)))
    return (x, dout, params), runs[0], runs[1]
