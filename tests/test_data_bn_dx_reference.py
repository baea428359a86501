"""CPU: tests/data_bn_dx_reference.py (the float64 restatement of the backward apply pass of data_bn, the yardstick of
tests/test_gpu_input_grad.py) against torch autograd through  x -> bone / motion transform -> oracle.stgcn.data_bn (training) ->
sum w*h,  everything in float64, k1..k3 formed from the same batch statistics by the formulas of bn_bwd_finalize.

The clips hold multiples of 1/8 below 8 in magnitude, so that the float32 transform the restatement recomputes is exact and equals
the float64 one autograd differentiates.  Tolerance: 1e-12 relative to max|dx| -- float64 rounding over fewer than 100 operations
per element.  Motion at T = 1 is the zero function: both sides must be exactly 0.  N = 5, so that the smallest case (T = 1, M = 1)
still has 5 samples per channel: with 2 the normalised values are +-1 whatever x is, the true gradient is of the size of eps and
max|dx| measures the cancellation, not the result."""
import numpy as np
import pytest
import torch

import data_bn_dx_reference as R
from oracle import stgcn as O


@pytest.mark.parametrize("stream", list(R.STREAMS))
@pytest.mark.parametrize("V", [25, 5])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_restatement_equals_autograd(stream, V, T, M):
    bone, motion = R.STREAMS[stream]
    parent = (R.ntu_parent() if V == 25 else R.HAND_PARENT) if bone else None
    N, C = 5, 3
    g = torch.Generator().manual_seed(1000 * V + 100 * T + 10 * M + len(stream))
    x = torch.randint(-63, 64, (N, C, T, V, M), generator=g).double() / 8
    p = {"data_bn.gamma": torch.rand(V * C, generator=g, dtype=torch.float64) + 0.5,
         "data_bn.beta": torch.randn(V * C, generator=g, dtype=torch.float64),
         "data_bn.moving_mean": torch.zeros(V * C, dtype=torch.float64), "data_bn.moving_var": torch.ones(V * C, dtype=torch.float64)}
    w = torch.randn(N * M, C, T, V, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    val = R.stream_values(xr, parent, motion)
    (O.data_bn(val, p, True) * w).sum().backward()
    dh = w.permute(1, 0, 2, 3).reshape(C, -1)                           # d loss / d h, CN rows [C][((n*M+m)*T+t)*V+v]
    assert torch.equal(R.clip_to_cn(R.cn_to_clip(dh, N, C, T, V, M)), dh)
    k1, k2, k3 = R.bwd_coefficients(val.detach(), R.cn_to_clip(dh, N, C, T, V, M), p["data_bn.gamma"], O.BN_EPS)
    dx, S = R.data_bn_dx(x.float(), dh, k1, k2, k3, parent, motion)
    assert dx.shape == x.shape and S.shape == x.shape and dx.dtype == torch.float64
    scale = xr.grad.abs().max().item()
    if motion and T == 1:
        assert scale == 0.0 and dx.abs().max().item() == 0.0 and S.abs().max().item() == 0.0
        return
    assert scale > 0
    assert (dx - xr.grad).abs().max().item() <= 1e-12 * scale
    assert (S >= dx.abs() * (1 - 1e-12)).all()


def test_a_self_pair_contributes_nothing():
    """joint 4 of the hand-made table is its own parent and nobody else's: dx there is exactly 0 and has no magnitude; the NTU root
    (joint 21) is its own parent too: what arrives at it (dh of that joint) reaches no dx element"""
    g = torch.Generator().manual_seed(3)
    N, C, T, V, M = 2, 3, 4, 5, 2
    x = torch.randn(N, C, T, V, M, generator=g)
    dh = torch.randn(C, N * M * T * V, generator=g)
    k = [torch.randn(V * C, generator=g) for _ in range(3)]
    for motion in (False, True):
        dx, S = R.data_bn_dx(x, dh, *k, R.HAND_PARENT, motion)
        assert dx[:, :, :, 4].abs().max().item() == 0.0 and S[:, :, :, 4].abs().max().item() == 0.0
        assert dx[:, :, :, :4].abs().min().item() > 0.0
    V, parent = 25, R.ntu_parent()
    assert parent[20] == 20 and sorted(np.nonzero(parent == 20)[0]) == [1, 2, 4, 8, 20]
    x = torch.randn(N, C, T, V, M, generator=g)
    dh = torch.randn(C, N * M * T * V, generator=g)
    k = [torch.randn(V * C, generator=g) for _ in range(3)]
    dx, _ = R.data_bn_dx(x, dh, *k, parent, True)
    dh2 = R.cn_to_clip(dh, N, C, T, V, M).clone()
    dh2[:, :, :, 20] = 7.0
    dx2, _ = R.data_bn_dx(x, R.clip_to_cn(dh2), *k, parent, True)
    assert torch.equal(dx, dx2)
