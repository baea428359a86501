"""GPU: every entry point of csrc/tattn.hip on operands that are views into larger allocations (tests/util.py: Launch, drive,
guarded_flat).  x, out, dout and dx are CN matrices [C][N T V] and the hidden activations / their gradients CN matrices [units][N T],
each with guard rows in front and behind and `pad` columns of margin at the right of every row; the gate, the parameters, the slabs and
the reduced gradient are flat ranges between guard elements.  Inputs are surrounded by NaN -- whatever reads the margin and lets it
reach a result shows --, outputs by a sentinel that has to survive.  Asserted per launch: the guards are untouched, the inputs are
unmodified, every output is finite, the padded run is bitwise the unpadded one, and both are bitwise what sar_amd.ops.tattn_forward /
tattn_backward give on plain NCHW tensors."""
import pytest
import torch

import tattn_cases as K
from util import Launch, drive

pytestmark = pytest.mark.gpu

RELU, SIGMOID = 0, 1


class Kept(Launch):
    KEEP_INPUTS = True


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cn(t):
    """(N, C, T, V) -> (C, N T V)"""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def layer(dev, case):
    """the five kernels of the layer and the two activation kernels, every buffer a guarded view"""
    from sar_amd import _lib as L
    from sar_amd import ops
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, T, V, hidden, _ = case
    (x, dout, params), _, _ = K.reference(case)
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    x, dout, params = f(x), f(dout), [f(p) for p in params]
    out0, saved0 = ops.tattn_forward(x, params)
    keep = {}
    dx0, grads0 = ops.tattn_backward(x, saved0, params, dout, keep=keep)
    a0, h1_0, dz1_0, dzL_0 = saved0[0], (saved0[1] if hidden else saved0[0].view(1, -1)), keep["dz_1"], keep["dz_L"].reshape(-1)
    n, u, nv = N * T, params[0].shape[1], N * T * V
    size = V * C * u + u
    z_src = torch.randn(u, n, generator=torch.Generator().manual_seed(2)).to(dev)

    def fn(g):
        lib, st = L.load(), stream_ptr()
        X, D, DZ1, H = g.inp(_cn(x)), g.inp(_cn(dout)), g.inp(dz1_0), g.inp(h1_0)
        k1, b1, a = g.flat_in(params[0]), g.flat_in(params[1]), g.flat_in(a0)
        h1, out, dx = g.out("h1", u, n), g.out("out", C, nv), g.out("dx", C, nv)
        z, zs, dh = g.out("relu", u, n), g.out("sigmoid", u, n), g.out("dact", u, n)
        for t in (z, zs, dh):
            t.copy_(z_src)
        nslab = lib.sar_tattn_wgrad_slabs(N, C, T, V)
        dzL, slab, grad1 = g.flat("dzL", n), g.flat("slab", nslab * size), g.flat("grad1", size)
        ld_x, ld_h = X.stride(0), h1.stride(0)
        assert ld_x == nv + g.pad == D.stride(0) == out.stride(0) == dx.stride(0) and ld_h == n + g.pad == DZ1.stride(0) == H.stride(0)
        sx = (T * V, ld_x)
        check(lib.sar_tattn_score_f32(ptr(X), *sx, ptr(k1), ptr(b1), N, C, T, V, u, RELU if hidden else SIGMOID, ptr(h1), ld_h, st), "score")
        check(lib.sar_tattn_scale_f32(ptr(X), *sx, ptr(a), N, C, T, V, ptr(out), *sx, st), "scale")
        check(lib.sar_tattn_dscore_f32(ptr(X), *sx, ptr(D), *sx, ptr(a), N, C, T, V, ptr(dzL), st), "dscore")
        check(lib.sar_tattn_wgrad_f32(ptr(X), *sx, ptr(DZ1), ld_h, N, C, T, V, u, ptr(slab), nslab, st), "wgrad")
        check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(grad1), st), "slab_reduce")
        check(lib.sar_tattn_dx_f32(ptr(D), *sx, ptr(a), ptr(k1), ptr(DZ1), ld_h, N, C, T, V, u, ptr(dx), *sx, st), "dx")
        check(lib.sar_tattn_act_f32(ptr(z), ld_h, u, n, RELU, st), "act relu")
        check(lib.sar_tattn_act_f32(ptr(zs), ld_h, u, n, SIGMOID, st), "act sigmoid")
        check(lib.sar_tattn_dact_f32(ptr(H), ld_h, ptr(dh), ld_h, u, n, st), "dact")
        for what, got, want in (("h1", h1, h1_0), ("out", out, _cn(out0)), ("dzL", dzL, dzL_0), ("dx", dx, _cn(dx0)),
                                ("grad1", grad1, torch.cat([grads0[0].reshape(-1), grads0[1].reshape(-1)])),
                                ("relu", z, torch.relu(z_src)), ("dact", dh, torch.where(h1_0 > 0, z_src, torch.zeros_like(z_src)))):
            g.ref(what, got, want, 0)
    return fn


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("case", K.SMALL, ids=K.case_id)
def test_every_kernel_between_guards(dev, case, pad):
    drive(dev, layer(dev, case), pad, launch=Kept)
