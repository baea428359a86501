"""The shared cases of the AdaptiveAdjacency tests: (N, C, T, V, K, Ce, seed).

How a case is drawn: at initialisation-sized weights the logits are flat (the per-column standard deviation is 0.01 to 0.03 at the
workload widths), the softmax is uniform and tests nothing.  So x and dA_eff are randn, the kernels randn / sqrt(C), phi.bias 0.1 randn,
A 0.3 rand, and theta.kernel is then rescaled so that the mean per-column standard deviation of the float64 logits is LOGIT_STD = 2;
S is linear in theta.kernel, so the scaling is exact (tests/test_adjattn_reference.py asserts it, and max |S| <= 40)."""
import functools

import torch

import adjattn_reference as R

LOGIT_STD = 2.0

LISTED = [
    (3, 5, 7, 25, 3, 2, 0),             # nothing a multiple of anything
    (2, 16, 40, 25, 3, 4, 0),
    (1, 3, 1, 25, 3, 1, 0),             # one frame, contraction length 1
    (2, 8, 5, 32, 2, 3, 0),             # V = 32, the limit
    (2, 8, 5, 1, 3, 2, 0),              # V = 1
    (5, 4, 33, 19, 1, 7, 0),            # K = 1, odd T: a last step of one frame, a dembed tile of one frame
    (1, 6, 130, 25, 3, 5, 0),
    (2, 64, 300, 25, 3, 16, 0),         # the contraction length of the workload, at batch 2: 2 400 steps in 5 slabs
    (2, 256, 75, 25, 3, 64, 0),         # 2 432 steps in 5 slabs
    (2, 4, 9, 31, 4, 1, 0),             # K = 4
    (16, 6, 12, 25, 3, 4, 0),           # for the slice test
]
# sizes at which csrc/adjattn.hip takes another path
EDGES = [
    (1, 4, 38, 25, 1, 27, 0),           # 27 * 19 = 513 steps: the first size with two slabs (257 + 256 steps); 54 tiles in 4 dembed chunks
    (2, 3, 32, 7, 2, 16, 0),            # 256 steps = 64 per wave, whole groups of 8; frames = exactly one dembed tile, 16 tiles = one chunk
    (1, 2, 3, 5, 1, 1, 0),              # 2 steps: waves 2 and 3 of the similarity have none, three waves of dembed have no tile
    (1, 5, 64, 6, 2, 9, 0),             # 288 steps = 72 per wave: every group of 8 whole; 18 tiles over 2 chunks: a third round that two waves take
]
CASES = LISTED + EDGES
SLICE, SLICE_N = LISTED[10], 4
SMALL = [LISTED[2], LISTED[4], EDGES[2]]      # the guard-band cases: the three smallest
WORKLOAD = (LISTED[7], LISTED[8])


def case_id(case):
    return "%dx%dx%dx%d-K%d-Ce%d" % tuple(case[:6])


def make_case(case):
    """(x, A, theta_kernel (C, K Ce), phi_kernel (C, K Ce), phi_bias (K Ce), dA_eff) in float64"""
    N, C, T, V, K, Ce, seed = case
    gen = torch.Generator().manual_seed(seed)
    r = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    x, dA_eff = r((N, C, T, V)), r((N, K, V, V))
    tk, pk = r((C, K * Ce)) / C ** 0.5, r((C, K * Ce)) / C ** 0.5
    pb = 0.1 * r((K * Ce,))
    A = 0.3 * torch.rand(K, V, V, generator=gen, dtype=torch.float64)
    if V > 1:
        tk = tk * (LOGIT_STD / R.column_std(R.forward(x, A, tk, pk, pb)[1]["S"]))
    return x, A, tk, pk, pb, dA_eff


QUANTITIES = ("A_eff", "dx", "dtheta_kernel", "dphi_kernel", "dphi_bias", "dA")


def run(inputs, dtype):
    """the restatement in `dtype` -> dict of A_eff, the gradients and the intermediates theta, phi (N, K Ce, T, V), S, P, dS, dtheta, dphi"""
    x, A, tk, pk, pb, dA_eff = (t.to(dtype) for t in inputs)
    A_eff, ctx = R.forward(x, A, tk, pk, pb)
    out = R.backward(ctx, dA_eff)
    out.update(A_eff=A_eff, theta=ctx["theta"], phi=ctx["phi"], S=ctx["S"], P=ctx["P"])
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, float64 run, float32 run), computed once and shared, never modified"""
    inputs = make_case(case)
    return inputs, run(inputs, torch.float64), run(inputs, torch.float32)
