"""The shared cases of the TemporalConv tests: (N, C, M, T, V, k, d, s, padding), the smallest that reach each branch of csrc/tconv.hip.
Inputs from a seeded generator: x, dout ~ N(0, 1), W ~ N(0, 1 / (k C)), bias ~ 0.5 N(0, 1): out has unit scale and no quantity is
ill-conditioned."""
import functools

import torch

import tconv_reference as R

PLAIN = (2, 8, 8, 12, 5, 3, 1, 1, "same")
TWO_SAMPLES = (3, 4, 4, 7, 5, 3, 2, 1, "same")          # 35 columns per sample: the second 32-column block of a tile is nearly empty
STGCN_S1 = (2, 64, 64, 13, 25, 9, 1, 1, "same")         # ST-GCN's own shapes, also compared with ops.conv_gemm / conv_wgrad
STGCN_S2 = (2, 64, 128, 12, 25, 9, 1, 2, "same")        # SAME (3, 4)
K1_S2 = (2, 8, 8, 10, 5, 1, 1, 2, "same")               # k = 1: also conv1x1_fwd on the even frames
STRIDE2 = (2, 8, 8, 13, 5, 5, 2, 2, "same")
ONE_ROW = (2, 33, 1, 6, 7, 3, 2, 1, "same")             # contraction tail of 1, one output row
TWO_SLABS = (5, 3, 2, 4, 5, 3, 1, 1, "same")            # 5 tiles: the smallest N at which sar_tconv_wgrad_slabs answers 2 (3 + 2 tiles)

CASES = [
    PLAIN,
    TWO_SAMPLES,
    STGCN_S1,
    STGCN_S2,
    (2, 5, 6, 5, 3, 3, 8, 1, "same"),                   # the dilation exceeds T: most taps read only padding
    (2, 3, 2, 1, 4, 5, 4, 1, "same"),
    (2, 3, 65, 6, 25, 5, 1, 1, "same"),                 # the first layer's 3 channels, a row tail of 1 past two 32-row blocks
    ONE_ROW,
    (2, 16, 16, 9, 25, 5, 2, 1, "same"),                # the 16-row branch of an MS-TCN block
    (2, 8, 8, 12, 33, 3, 2, 1, "same"),                 # V over 32
    (2, 8, 8, 12, 1, 3, 2, 1, "same"),                  # V = 1
    (2, 8, 8, 12, 5, 5, 2, 2, "same"),                  # stride 2 with dilation: T even and odd, both padding rules
    STRIDE2,
    (2, 8, 8, 12, 5, 5, 2, 2, 4),
    (2, 8, 8, 13, 5, 3, 3, 2, 3),
    (2, 6, 6, 9, 5, 2, 1, 1, "same"),                   # even k
    (2, 6, 6, 9, 5, 4, 3, 2, "same"),
    K1_S2,
    TWO_SLABS,
]
GUARDED = [TWO_SAMPLES, STRIDE2, ONE_ROW]               # the guard-band cases
SLICE, SLICE_N = (16, 8, 8, 13, 5, 5, 2, 2, "same"), 4   # batch independence: every 4-sample slice of the 16-sample run
QUANTITIES = ("out", "dx", "dW", "dbias")


def case_id(case):
    return "%dx%d-%dx%dx%d-k%dd%ds%d-%s" % case


def make_case(case):
    """(x, W (k, 1, C, M), bias, dout) in float64"""
    N, C, M, T, V, k, d, s, padding = case
    T_out, _ = R.geometry(T, k, s, d, padding)
    gen = torch.Generator().manual_seed(1234)
    r = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    return r((N, C, T, V)), r((k, 1, C, M)) / (k * C) ** 0.5, 0.5 * r((M,)), r((N, M, T_out, V))


def run(case, inputs, dtype):
    x, W, bias, dout = (t.to(dtype) for t in inputs)
    _, _, _, T, _, k, d, s, padding = case
    T_out, pad = R.geometry(T, k, s, d, padding)
    out = R.forward(x, W, bias, s, d, pad, T_out)
    dx, dW, dbias = R.backward(x, W, dout, s, d, pad)
    return dict(out=out, dx=dx, dW=dW, dbias=dbias)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, float64 run, float32 run), computed once and shared, never modified"""
    inputs = make_case(case)
    return inputs, run(case, inputs, torch.float64), run(case, inputs, torch.float32)
