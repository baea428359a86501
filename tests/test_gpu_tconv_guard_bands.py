"""GPU: every entry point of csrc/tconv.hip on operands that are views into larger allocations (tests/util.py: Launch, drive).
x, dout, out and dx are CN matrices [channels][ld] with guard rows in front and behind and `pad` columns of margin at the right of every
row, handed to the kernels as (pointer, s_n = T V, s_c = ld); the kernel, its (k, M, C) image, the bias, the slabs and the reduced weight
gradient are flat ranges between guard elements.  Inputs are surrounded by NaN -- whatever reads the margin and lets it reach a result
shows --, outputs by a sentinel that has to survive.  Asserted per launch: the guards are untouched, the inputs are unmodified, every
output is finite, the padded run is bitwise the unpadded one, and both are bitwise what sar_amd.ops.tconv_* give on plain NCHW tensors."""
import pytest
import torch

import tconv_cases as K
import tconv_reference as R
from util import Launch, drive, to_cn

pytestmark = pytest.mark.gpu


class Kept(Launch):
    KEEP_INPUTS = True


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def layer(dev, case):
    """the three entry points (and the slab sum) of the layer, every buffer a guarded view"""
    from sar_amd import _lib as L
    from sar_amd import ops
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, M, T, V, k, d, s, padding = case
    T_out, pad = R.geometry(T, k, s, d, padding)
    x, W, b, dout = (t.to(torch.float32).to(dev).contiguous() for t in K.reference(case)[0])
    out0 = ops.tconv_forward(x, W, b, s, d, pad, T_out)
    dx0 = ops.tconv_backward_data(dout, W, T, s, d, pad)
    dW0, db0 = ops.tconv_wgrad(x, dout, k, s, d, pad)
    Wt0 = torch.empty((k, M, C), dtype=torch.float32, device=dev)
    ops.transpose(W, Wt0, k, C, M)
    n_in, n_out, size = N * T * V, N * T_out * V, k * C * M + M

    def fn(g):
        lib, st = L.load(), stream_ptr()
        X, D = g.inp(to_cn(x)), g.inp(to_cn(dout))
        Wg, Wtg, bg = g.flat_in(W), g.flat_in(Wt0), g.flat_in(b)
        out, dx = g.out("out", M, n_out), g.out("dx", C, n_in)
        nslab = lib.sar_tconv_wgrad_slabs(N, C, M, T_out, V)
        slab, flat = g.flat("slab", nslab * size), g.flat("dW|dbias", size)
        assert X.stride(0) == n_in + g.pad == dx.stride(0) and D.stride(0) == n_out + g.pad == out.stride(0)
        xs, os_ = (T * V, n_in + g.pad), (T_out * V, n_out + g.pad)
        check(lib.sar_tconv_fwd_f32(ptr(X), *xs, ptr(Wg), ptr(bg), N, C, M, T, T_out, V, k, d, s, pad, ptr(out), *os_, st), "fwd")
        check(lib.sar_tconv_bwd_data_f32(ptr(D), *os_, ptr(Wtg), N, C, M, T, T_out, V, k, d, s, pad, ptr(dx), *xs, st), "bwd_data")
        check(lib.sar_tconv_wgrad_f32(ptr(X), *xs, ptr(D), *os_, N, C, M, T, T_out, V, k, d, s, pad, ptr(slab), nslab, st), "wgrad")
        check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(flat), st), "slab_reduce")
        g.ref("out", out, to_cn(out0), 0)
        g.ref("dx", dx, to_cn(dx0), 0)
        g.ref("dW|dbias", flat, torch.cat([dW0.reshape(-1), db0]), 0)
    return fn


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("case", K.GUARDED, ids=K.case_id)
def test_every_kernel_between_guards(dev, case, pad):
    drive(dev, layer(dev, case), pad, launch=Kept)
