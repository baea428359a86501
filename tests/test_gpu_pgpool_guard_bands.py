"""GPU: every kernel of csrc/pgpool.hip on operands that are views into larger allocations (tests/util.py: guarded, drive,
assert_guards_untouched).  The CN operands x, q, dq / dl and dx are (rows, B P) views with guard rows in front and behind and `pad`
columns of margin at the right of every row; the per-sample and parameter tensors are flat ranges between guard elements.  Inputs
are surrounded by NaN -- whatever reads the margin and lets it reach a result shows --, outputs by a sentinel that has to survive.
Asserted per launch: the guards are untouched, every output is finite, the padded run is bitwise the unpadded one, and both are
bitwise what sar_amd.ops.pgpool_forward / pgpool_backward give on plain tensors."""
import pytest
import torch

import pgpool_reference as R
from util import NAN, drive, guarded_flat

pytestmark = pytest.mark.gpu

SHAPES = [(3, 40, 37, 24), (2, 64, 130, 33)]      # the first two shapes of tests/test_gpu_pgpool.py
CLAMP_FILL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(dev, shape, regime):
    B, C, P, J = shape
    x, cen, var = R.make_case(regime, B, C, P, J, 0)
    g = torch.Generator().manual_seed(1)
    dz = torch.randn(B, C, J, generator=g)
    dA = torch.randn(B, J, J, generator=g)
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    return f(x.permute(1, 0, 2).reshape(C, B * P)), f(cen), f(var), f(dz), f(dA)


def layer(dev, shape, regime):
    """the twelve entry points in the order of ops.pgpool_forward / pgpool_backward, every buffer a guarded view"""
    from sar_amd import _lib as L
    from sar_amd import ops
    from sar_amd._lib import check, ptr, stream_ptr
    B, C, P, J = shape
    X, cen, var, dz, dA = _case(dev, shape, regime)
    zn0, A0, saved0 = ops.pgpool_forward(X, B, P, cen, var)
    dX0, dcen0, dvar0 = torch.empty_like(X), torch.empty_like(cen), torch.empty_like(var)
    ops.pgpool_backward(X, B, P, cen, zn0, saved0, dz, dA, dX0, dcen0, dvar0)

    def fn(g):
        lib, st = L.load(), stream_ptr()
        inp = lambda t: guarded_flat(t, NAN, dev)[0]
        x, cen_g, var_g, dz_g, dA_g = g.inp(X), inp(cen), inp(var), inp(dz), inp(dA)
        W = lib.sar_pgpool_clamp_words(J)
        clamp, g.clamp_whole = guarded_flat(B * P * W, CLAMP_FILL, dev, dtype=torch.int32)
        q, dq, dx = g.out("q", J, B * P), g.out("dq", J, B * P), g.out("dx", C, B * P)
        n = B * C * J
        tab, S, zn, A, qs, n2 = g.flat("tab", 4 * C * J), g.flat("zp", n), g.flat("zn", n), g.flat("A", B * J * J), g.flat("qs", B * J), g.flat("n2", B * C)
        dzn, dS, dqs, M2 = g.flat("dzn_M1", n), g.flat("dS", n), g.flat("dqs_M0", B * J), g.flat("M2", n)
        dcen, dvar = g.flat("dcenters", C * J), g.flat("dvariance", C * J)
        ld = x.stride(0)
        assert ld == B * P + g.pad and q.stride(0) == ld and dq.stride(0) == ld and dx.stride(0) == ld
        check(lib.sar_pgpool_prep_f32(ptr(cen_g), ptr(var_g), C, J, ptr(tab), st), "prep")
        check(lib.sar_pgpool_assign_f32(ptr(x), ld, B, P, C, J, ptr(cen_g), ptr(tab), ptr(q), ld, ptr(clamp), st), "assign")
        check(lib.sar_pgpool_moment_f32(ptr(x), ld, ptr(q), ld, B, P, C, J, 0, ptr(S), st), "moment")
        check(lib.sar_pgpool_rowsum_f32(ptr(q), ld, B, P, J, ptr(qs), st), "rowsum")
        check(lib.sar_pgpool_normalize_f32(ptr(S), ptr(qs), ptr(cen_g), ptr(tab), B, C, J, ptr(zn), ptr(n2), st), "normalize")
        check(lib.sar_pgpool_gram_f32(ptr(zn), B, C, J, ptr(A), st), "gram")
        check(lib.sar_pgpool_gram_bwd_f32(ptr(zn), ptr(dz_g), ptr(dA_g), B, C, J, ptr(dzn), st), "gram_bwd")
        check(lib.sar_pgpool_normalize_bwd_f32(ptr(dzn), ptr(zn), ptr(S), ptr(n2), ptr(qs), ptr(cen_g), ptr(tab), B, C, J, ptr(dS), ptr(dqs),
                                               st), "normalize_bwd")
        check(lib.sar_pgpool_dq_f32(ptr(x), ld, ptr(dS), ptr(dqs), B, P, C, J, ptr(dq), ld, st), "dq")
        check(lib.sar_pgpool_softmax_bwd_f32(ptr(q), ld, ptr(clamp), B, P, J, ptr(dq), ld, st), "softmax_bwd")
        check(lib.sar_pgpool_dx_f32(ptr(x), ld, ptr(dS), ptr(q), ld, ptr(dq), ld, ptr(tab), B, P, C, J, ptr(dx), ld, st), "dx")
        check(lib.sar_pgpool_rowsum_f32(ptr(dq), ld, B, P, J, ptr(dqs), st), "rowsum")
        check(lib.sar_pgpool_moment_f32(ptr(x), ld, ptr(dq), ld, B, P, C, J, 0, ptr(dzn), st), "moment")
        check(lib.sar_pgpool_moment_f32(ptr(x), ld, ptr(dq), ld, B, P, C, J, 1, ptr(M2), st), "moment")
        check(lib.sar_pgpool_param_grad_f32(ptr(dqs), ptr(dzn), ptr(M2), ptr(dS), ptr(qs), ptr(S), ptr(cen_g), ptr(tab), B, C, J, ptr(dcen),
                                            ptr(dvar), st), "param_grad")
        g.clamp = clamp
        for what, got, want in (("q", q, saved0[0]), ("zn", zn, zn0), ("A_out", A, A0), ("zp", S, saved0[2]), ("qs", qs, saved0[3]),
                                ("dx", dx, dX0), ("dcenters", dcen, dcen0), ("dvariance", dvar, dvar0)):
            g.ref(what, got.reshape(-1) if got.dim() == 1 else got, want.reshape(-1) if got.dim() == 1 else want, 0)
    return fn


@pytest.mark.parametrize("pad", [1, 7, 64])
@pytest.mark.parametrize("regime", ["spread", "init"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kernel_between_guards(dev, shape, regime, pad):
    tight, padded = drive(dev, layer(dev, shape, regime), pad)
    for g in (tight, padded):
        k = 8
        n = g.clamp.numel()
        assert bool((g.clamp_whole[:k] == CLAMP_FILL).all()) and bool((g.clamp_whole[k + n:] == CLAMP_FILL).all()), "clamp words: guards written"
        assert not bool(g.clamp.any()), "the clamp held nowhere in these cases"
    assert torch.equal(tight.clamp, padded.clamp)
