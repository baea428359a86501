"""The restatement of ProjectionGraphPool (tests/pgpool_reference.py) pinned before the GPU tests rely on it: its hand-written
backward pass against central finite differences and against torch autograd of the literal formulation (which materialises z), the
structure of its outputs, and the layer's initialisation."""
import math

import numpy as np
import pytest
import torch

import pgpool_reference as R

SHAPES = [(2, 5, 7, 4), (2, 8, 12, 6)]      # (B, C, P, J)


def _case(shape, seed):
    B, C, P, J = shape
    x, cen, var = R.make_case("spread", B, C, P, J, seed)
    g = torch.Generator().manual_seed(seed + 100)
    dz = torch.randn(B, C, J, generator=g, dtype=torch.float64)
    dA = torch.randn(B, J, J, generator=g, dtype=torch.float64)      # not symmetric
    return [x, cen, var], dz, dA


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_match_autograd_of_the_literal_formulation(shape):
    args, dz, dA = _case(shape, 0)
    zn, A, ctx = R.pool_forward(*args)
    leaves = [t.clone().requires_grad_(True) for t in args]
    z_lit, A_lit = R.literal(*leaves)
    assert (zn - z_lit).abs().max().item() <= 1e-13 and (A - A_lit).abs().max().item() <= 1e-13
    want = torch.autograd.grad((z_lit * dz).sum() + (A_lit * dA).sum(), leaves)
    for name, got, ref in zip(("dx", "dcenters", "dvariance"), R.pool_backward(ctx, dz, dA), want):
        err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        assert err <= 1e-11, (name, err)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_central_finite_differences(shape):
    args, dz, dA = _case(shape, 1)
    _, _, ctx = R.pool_forward(*args)
    grads = R.pool_backward(ctx, dz, dA)

    def f(a):
        zn, A, _ = R.pool_forward(*a)
        return ((zn * dz).sum() + (A * dA).sum()).item()

    h = 1e-6
    rng = np.random.default_rng(3)
    for i, (a, ga) in enumerate(zip(args, grads)):
        flat = a.view(-1)
        for k in rng.choice(flat.numel(), size=min(20, flat.numel()), replace=False):
            old = flat[k].item()
            flat[k] = old + h
            fp = f(args)
            flat[k] = old - h
            fm = f(args)
            flat[k] = old
            fd, an = (fp - fm) / (2 * h), ga.reshape(-1)[k].item()
            assert abs(fd - an) <= 2e-6 * max(1.0, abs(fd)), (i, int(k), fd, an)


@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_are_unit_rows_and_a_symmetric_gram_matrix(shape):
    args, _, _ = _case(shape, 2)
    zn, A, ctx = R.pool_forward(*args)
    B, C, P, J = shape
    assert tuple(zn.shape) == (B, C, J) and tuple(A.shape) == (B, J, J)
    assert ((zn * zn).sum(-1) - 1).abs().max().item() <= 1e-12          # l2_normalize over the last axis: sum_j zn^2 = 1
    assert torch.equal(A, A.transpose(1, 2).contiguous()) or (A - A.transpose(1, 2)).abs().max().item() <= 1e-15
    assert (torch.diagonal(A, dim1=1, dim2=2).sum(-1) - C).abs().max().item() <= 1e-11      # trace = one per channel
    assert (ctx["q"].sum(-1) - 1).abs().max().item() <= 1e-12


def test_autograd_function_matches_the_plain_backward():
    args, dz, dA = _case(SHAPES[1], 4)
    leaves = [t.clone().requires_grad_(True) for t in args]
    zn, A = R.Pool.apply(*leaves)
    torch.autograd.backward([zn, A], [dz, dA])
    _, _, ctx = R.pool_forward(*args)
    for a, want in zip(leaves, R.pool_backward(ctx, dz, dA)):
        assert torch.equal(a.grad, want.reshape(a.shape))


def test_float32_run_of_the_same_code_is_the_band():
    """the same functions in float32: close to float64 on spread-out inputs, and the dtype follows the inputs"""
    args, dz, dA = _case(SHAPES[1], 5)
    zn, A, ctx = R.pool_forward(*args)
    zn32, A32, ctx32 = R.pool_forward(*[t.float() for t in args])
    assert zn32.dtype == torch.float32 and (zn32.double() - zn).abs().max().item() <= 1e-5
    for got, want in zip(R.pool_backward(ctx32, dz.float(), dA.float()), R.pool_backward(ctx, dz, dA)):
        assert got.dtype == torch.float32
        assert (got.double() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


@pytest.mark.parametrize("regime,shape", [("spread", (3, 40, 37, 24)), ("init", (3, 40, 37, 24)), ("init", (2, 64, 130, 33))])
def test_regimes_meet_the_preconditions_of_the_gpu_tests(regime, shape):
    B, C, P, J = shape
    _, _, ctx = R.pool_forward(*R.make_case(regime, B, C, P, J, 0))
    qs_min, d_min, n2_min = R.preconditions(ctx)
    assert qs_min >= 1e-3 and d_min > 1e-9 and n2_min >= 1e-6


def test_init_regime_is_glorot_uniform():
    from sar_amd.stpgcn import glorot_uniform
    limit = R.glorot_limit(256, 512)
    assert abs(limit - math.sqrt(6.0 / (256 + 512 * 256))) < 1e-15 and abs(limit - 0.00676) < 1e-5
    w = glorot_uniform((1, 256, 1, 512), torch.Generator().manual_seed(0))
    assert w.abs().max().item() <= limit and w.abs().max().item() > 0.99 * limit
    _, cen, var = R.make_case("init", 1, 256, 2, 512, 0)
    assert cen.abs().max().item() <= limit and var.abs().max().item() <= limit
