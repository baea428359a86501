"""GPU: every kernel of csrc/gpool.hip on operands that are views into larger allocations (tests/util.py: guarded, drive,
assert_guards_untouched).  x, out, dout and dx are CN matrices [C][N T W] with guard rows in front and behind and `pad` columns of
margin at the right of every row, passed by their two strides (s_n = T W, s_c = ld); the per-sample tensors, the partial sums and
the parameter are flat ranges between guard elements.  Inputs are surrounded by NaN -- whatever reads the margin and lets it reach a
result shows --, outputs by a sentinel that has to survive.  Asserted per launch: the guards are untouched, every output is finite,
the padded run is bitwise the unpadded one, and both are bitwise what sar_amd.ops.gpool_forward / gpool_backward give on plain NCHW
tensors."""
import pytest
import torch

import gpool_reference as R
from util import NAN, drive, guarded_flat

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 25, 3, 0.5), (2, 6, 5, 33, 4, 0.7), (2, 3, 300, 25, 3, 0.5)]      # shapes of tests/test_gpu_gpool.py
INT_FILL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cn(t):
    """(N, C, T, W) -> (C, N T W)"""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def layer(dev, shape):
    """the eleven entry points in the order of ops.gpool_forward / gpool_backward, every buffer a guarded view"""
    from sar_amd import _lib as L
    from sar_amd import ops
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, T, V, K, keeprate = shape
    x, A, p, dout, dA_out = (t.float().to(dev).contiguous() for t in R.make_case(shape, 0))
    keep = dout.shape[3]
    out0, A_out0, saved0 = ops.gpool_forward(x, A, p, keeprate)
    dx0, dp0, dA0 = ops.gpool_backward(x, A, saved0, dout, dA_out)

    def fn(g):
        lib, st = L.load(), stream_ptr()
        inp = lambda t: guarded_flat(t, NAN, dev)[0]
        X, D, A_g, p_g, dAo_g = g.inp(_cn(x)), g.inp(_cn(dout)), inp(A), inp(p), inp(dA_out)
        out, dx = g.out("out", C, N * T * keep), g.out("dx", C, N * T * V)
        ng = lib.sar_gpool_groups(C, T)
        ph, norm, part, y, sv = g.flat("ph", C * T), g.flat("norm", 2), g.flat("part", N * ng * V), g.flat("y", N * V), g.flat("s", N * keep)
        A_out, dspart, dy, dphp = g.flat("A_out", N * K * keep * keep), g.flat("dspart", N * ng * keep), g.flat("dy", N * V), g.flat("dphp", N * C * T)
        dph, dp, dA = g.flat("dph", C * T), g.flat("dp", C * T), g.flat("dA", N * K * V * V)
        idx, g.idx_whole = guarded_flat(N * keep, INT_FILL, dev, dtype=torch.int32)
        pos, g.pos_whole = guarded_flat(N * V, INT_FILL, dev, dtype=torch.int32)
        ld_x, ld_o = X.stride(0), out.stride(0)
        assert ld_x == N * T * V + g.pad == dx.stride(0) and ld_o == N * T * keep + g.pad == D.stride(0)
        sx, so = (T * V, ld_x), (T * keep, ld_o)
        check(lib.sar_gpool_prep_f32(ptr(p_g), C * T, ptr(ph), ptr(norm), st), "prep")
        check(lib.sar_gpool_score_f32(ptr(X), *sx, ptr(ph), N, C, T, V, ptr(part), st), "score")
        check(lib.sar_gpool_select_f32(ptr(part), N, C, T, V, keep, ptr(y), ptr(idx), ptr(sv), ptr(pos), st), "select")
        check(lib.sar_gpool_gather_f32(ptr(X), *sx, ptr(idx), ptr(sv), N, C, T, V, keep, ptr(out), *so, st), "gather")
        check(lib.sar_gpool_adj_f32(ptr(A_g), ptr(idx), N, K, V, keep, ptr(A_out), st), "adj")
        check(lib.sar_gpool_ds_f32(ptr(X), *sx, ptr(D), *so, ptr(idx), N, C, T, V, keep, ptr(dspart), st), "ds")
        check(lib.sar_gpool_dy_f32(ptr(dspart), ptr(sv), ptr(idx), N, C, T, V, keep, ptr(dy), st), "dy")
        check(lib.sar_gpool_dx_f32(ptr(X), *sx, ptr(D), *so, ptr(pos), ptr(sv), ptr(dy), ptr(ph), N, C, T, V, keep, ptr(dx), *sx, ptr(dphp),
                                   st), "dx")
        check(lib.sar_gpool_dp_f32(ptr(dphp), ptr(ph), ptr(norm), N, C * T, ptr(dph), ptr(dp), st), "dp")
        check(lib.sar_gpool_adj_bwd_f32(ptr(A_g), ptr(dAo_g), ptr(idx), ptr(pos), N, K, V, keep, ptr(dA), st), "adj_bwd")
        g.idx, g.pos = idx, pos
        for what, got, want in (("out", out, _cn(out0)), ("dx", dx, _cn(dx0)), ("A_out", A_out, A_out0), ("y", y, saved0[2]), ("s", sv, saved0[3]),
                                ("dp", dp, dp0), ("dA", dA, dA0)):
            g.ref(what, got.reshape(-1) if got.dim() == 1 else got, want.reshape(-1) if got.dim() == 1 else want, 0)
    return fn, saved0


@pytest.mark.parametrize("pad", [1, 7, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kernel_between_guards(dev, shape, pad):
    fn, saved0 = layer(dev, shape)
    tight, padded = drive(dev, fn, pad)
    k = 8
    for g in (tight, padded):
        for whole, live, want in ((g.idx_whole, g.idx, saved0[0]), (g.pos_whole, g.pos, saved0[1])):
            n = live.numel()
            assert bool((whole[:k] == INT_FILL).all()) and bool((whole[k + n:] == INT_FILL).all()), "index words: guards written"
            assert torch.equal(live, want.reshape(-1))
