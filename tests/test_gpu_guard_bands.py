"""Guard bands for the fp32 kernels behind the C ABI ("The leading-dimension contract"): every operand is a view into a
larger allocation -- ld = n + pad columns per row, 4 rows in front and 2 behind -- whose every other element holds a known fill:
NaN around inputs, -7.25 around outputs, 0xA5 around mask bytes.  Each kernel runs tight (pad = 0), with pad = 4 (rows stay
16-byte aligned: the vector paths) and with pad = 7 (the scalar paths); after each launch

  1. the live region meets the float64 bar of the kernel's own parity test (tolerances and references are those of
     test_gpu_stgcn_kernels.py, test_gpu_adjacency.py, test_gpu_stgcn_ta.py, test_gpu_stgin.py, test_gpu_stpgcn.py and
     test_gpu_conv2d_kernels.py, restated on the same seeded inputs);
  2. the live region is bitwise the tight launch's (a kernel that picks another summation order for a padded ld says so below);
  3. every guard element of every output still holds its fill, bit for bit;
  4. every output and every reduction partial is finite: no NaN of an input's padding reached a result;
  5. where the ABI rejects the leading dimension, the call raises (or relu_mask returns None) and the outputs hold only the fill.

The guards are part of the operand's own allocation, so a stray access shows as a failed assertion, never as a fault.

Rectangular and odd-sized 2-D cases (tests/conv2d_rect_cases.py): groups A and E whole, one case each of B, C and F.  Worst error over
the 2-D cases of this file, MEASURED on an MI355X, every launch bitwise equal to the tight one: A masked data gradient 5.2e-7, its sums
2.6e-7 / 3.7e-7, with the compact aux 4.4e-7; E max-pool 4.7e-8 forward, 1.3e-7 backward, sums 1.1e-7 / 1.4e-7; B, C, F through
test_conv2d_forward_data_and_weight_gradient: forward 3.7e-7, weight gradient 4.4e-7, data gradient 8.8e-7."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv2d_rect_cases as RC
from oracle import stgcn as O
from util import NAN, SENTINEL, Launch, drive, guarded, guarded_flat, mask_bytes, rejected, rel_err, to_cn

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # the per-kernel bar (tests/test_gpu_stgcn_kernels.py)
PADS = [4, 7]
FRONT, BACK, KFLAT = 4, 2, 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def cn(x):
    """(B, C, T, V) or (B, C, H, W) -> CN matrix [C][B * rest]"""
    return x.permute(1, 0, 2, 3).reshape(x.shape[1], -1).contiguous()


def _A():
    from oracle.graph import spatial_adjacency
    return torch.tensor(spatial_adjacency().astype(np.float32))


@functools.lru_cache(maxsize=None)
def _tables(transpose=False):
    from sar_amd import ops
    from oracle.graph import spatial_adjacency
    return ops.GraphTables(spatial_adjacency().astype(np.float32), torch.device("cuda:0"), transpose)


def _transposed(dev, w, batch, R, Cc):
    """the weight operand of a data gradient (ops.transpose, as the parity tests build it)"""
    from sar_amd import ops
    out = torch.empty((batch, Cc, R), device=dev)
    ops.transpose(w.float().to(dev).contiguous(), out, batch, R, Cc)
    return out


# ------------------------------------------------------------------------------------------------ conv_gemm / conv_wgrad: graph
GRAPH_SHAPES = [(3, 3, 64, 13), (2, 40, 72, 8)]


@functools.lru_cache(maxsize=None)
def graph_case(B, cin, f, T):
    """inputs and float64 results of GraphConvTD (tests/test_gpu_stgcn_kernels.py: test_graph_conv_forward_and_stats,
    test_graph_conv_gradients), computed once and never modified"""
    g = torch.Generator().manual_seed(7 * cin + f + 1000 * B)
    x = torch.randn(B, cin, T, 25, generator=g).double().requires_grad_(True)
    kernel = (torch.randn(1, 1, cin, 3 * f, generator=g) * 0.1).double().requires_grad_(True)
    bias = (torch.randn(3 * f, generator=g) * 0.1).double().requires_grad_(True)
    dout = torch.randn(B, f, T, 25, generator=g)
    y = O.graph_conv_td(x, kernel, bias, _A().double())
    gx, gk, gb = torch.autograd.grad(y, (x, kernel, bias), dout.double())
    n = B * T * 25
    extra = dict(add=torch.randn(cin, n, generator=g), u=torch.randn(cin, n, generator=g), mean=0.1 * torch.randn(cin, generator=g),
                 keep=torch.rand(cin, n, generator=g) > 0.4, compact=torch.randn(cin, B * ((T + 1) // 2) * 25, generator=g),
                 gamma=1 + 0.1 * torch.randn(f, generator=g), beta=0.1 * torch.randn(f, generator=g))
    return dict(x=x.detach(), kernel=kernel.detach(), bias=bias.detach(), dout=dout, y=y.detach(), gx=gx, gk=gk, gb=gb, **extra)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T", GRAPH_SHAPES)
def test_graph_conv_forward_with_stats(dev, B, cin, f, T, pad):
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n = B * T * 25
    W, bias = c["kernel"].float().to(dev), c["bias"].float().to(dev)

    def fn(g):
        out = g.out("out", f, n)
        r = ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["x"])), out, W, f, 3 * f, B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f, taps=3,
                          bias=bias, tables=_tables(), epi=L.SAR_EPI_STATS)
        g.part("stats", r[0])
        z = lambda: torch.empty(f, device=dev)
        mean, rstd, scale, shift = z(), z(), z(), z()
        ops.bn_finalize(r[0], r[1], f, n, 1e-3, 0.99, True, c["gamma"].to(dev), c["beta"].to(dev), torch.zeros(f, device=dev),
                        torch.ones(f, device=dev), mean, rstd, scale, shift)
        g.ref("graph forward", out, to_cn(c["y"]), TOL)
        g.ref("mean of the epilogue partials", mean, c["y"].mean(dim=(0, 2, 3)), TOL)
        g.ref("rstd of the epilogue partials", rstd, torch.rsqrt(c["y"].var(dim=(0, 2, 3), unbiased=False) + 1e-3), TOL)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("epi", ["none", "add"])
@pytest.mark.parametrize("B,cin,f,T", GRAPH_SHAPES)
def test_graph_data_gradient(dev, B, cin, f, T, epi, pad):
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n = B * T * 25
    gT = _transposed(dev, c["kernel"], 1, cin, 3 * f).view(3 * f, cin)

    def fn(g):
        dx = g.out("dx", cin, n)
        kw = dict(epi=L.SAR_EPI_ADD, aux=g.inp(c["add"])) if epi == "add" else {}
        ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), dx, gT, f * cin, cin, B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3,
                      tables=_tables(True), **kw)
        g.ref("graph data gradient (%s)" % epi, (lambda: dx.cpu() - c["add"]) if epi == "add" else dx, to_cn(c["gx"]), TOL)
    drive(dev, fn, pad)


def _gated(dev, B, cin, f, T):
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n = B * T * 25
    gT = _transposed(dev, c["kernel"], 1, cin, 3 * f).view(3 * f, cin)
    args = dict(B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3, tables=_tables(True))

    def plain(g):
        out = g.out("plain", cin, n)
        ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), out, gT, f * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(c["add"]), **args)
        return out

    def gated(g):
        out = g.out("gated", cin, n)
        u = g.inp(c["u"])
        pm = ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), out, gT, f * cin, cin, epi=L.SAR_EPI_ADD_GATE, aux=g.inp(c["add"]),
                           aux2=u, aux_mask=g.mask("keep", cin, n, c["keep"]), aux_mean=c["mean"].to(dev), **args)
        return out, pm
    return c, n, plain, gated


@pytest.mark.parametrize("pad", PADS)
def test_graph_data_gradient_gated_epilogue(dev, pad):
    """test_graph_data_gradient_gated_epilogue_f32 with aux, aux2 and the mask bytes guarded.  ld_aux2 % 4 != 0 (pad = 7) is
    rejected (csrc/conv_gemm.hip validate(): SAR_EPI_ADD_GATE), and so is every ld at (3, 3, 64, 13): M % 8 and n % 4 both fail."""
    B, cin, f, T = 2, 40, 72, 8
    c, n, plain, gated = _gated(dev, B, cin, f, T)
    if pad % 4:
        rejected(dev, lambda g: gated(g), pad)
        return

    def fn(g):
        p = plain(g)
        out, pm = gated(g)
        g.part("gate", pm[0])
        want = lambda: torch.where(c["keep"].to(dev), p, torch.zeros_like(p))
        g.ref("gated == ADD gated afterwards", out, want, 0)
        g.ref("gated data gradient", out, torch.where(c["keep"], to_cn(c["gx"]) + c["add"].double(), torch.zeros(1, dtype=torch.float64)), TOL)
        g.ref("sum out", lambda: pm[0].double().sum(dim=1)[:, 0], lambda: want().double().sum(dim=1), 1e-6)
        g.ref("sum out (aux2 - mean)", lambda: pm[0].double().sum(dim=1)[:, 1],
              lambda: (want().double().cpu() * (c["u"].double() - c["mean"].double().view(-1, 1))).sum(dim=1), 1e-6)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", [0] + PADS)
def test_graph_data_gradient_gated_epilogue_is_rejected_at_three_channels(dev, pad):
    _, _, _, gated = _gated(dev, 3, 3, 64, 13)
    rejected(dev, lambda g: gated(g), pad)


@pytest.mark.parametrize("pad", PADS)
def test_graph_data_gradient_even_frame_skip_add(dev, pad):
    """SAR_GRAPH_AUX_EVEN_FRAMES at (1, 3, 64, 7): the compact aux (4 of 7 frames) is a guarded view of its own, shorter, rows"""
    from sar_amd import ops, _lib as L
    B, cin, f, T = 1, 3, 64, 7
    c = graph_case(B, cin, f, T)
    n, Ta = B * T * 25, (T + 1) // 2
    full = torch.zeros(cin, B, T, 25)
    full[:, :, 0::2] = c["compact"].view(cin, B, Ta, 25)
    full = full.reshape(cin, n)
    gT = _transposed(dev, c["kernel"], 1, cin, 3 * f).view(3 * f, cin)
    args = dict(B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3, tables=_tables(True), epi=L.SAR_EPI_ADD)

    def fn(g):
        want, got = g.out("interleaved", cin, n), g.out("compact", cin, n)
        ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), want, gT, f * cin, cin, aux=g.inp(full), **args)
        ops.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), got, gT, f * cin, cin, aux=g.inp(c["compact"]), aux_even_frames=True, **args)
        g.ref("compact == zero-interleaved", got, want, 0)
        g.ref("data gradient + even-frame skip", got, to_cn(c["gx"]) + full.double(), TOL)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T", GRAPH_SHAPES + [(1, 3, 64, 7)])
def test_graph_weight_gradient(dev, B, cin, f, T, pad):
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    wsize, bsize = cin * 3 * f, 3 * f

    def fn(g):
        flat = g.flat("dW | dbias", wsize + bsize)
        ops.conv_wgrad(L.SAR_CONV_GRAPH, g.inp(to_cn(c["x"])), g.inp(to_cn(c["dout"])), flat, B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f,
                       taps=3, tables=_tables(), w_stride_tap=f, w_stride_c=3 * f, wsize=wsize, bsize=bsize)
        g.ref("graph dW", lambda: flat[:wsize].cpu().view(1, 1, cin, 3 * f), c["gk"], TOL)
        g.ref("graph dbias", lambda: flat[wsize:], c["gb"], TOL)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ conv_gemm / conv_wgrad: temporal
@functools.lru_cache(maxsize=None)
def temporal_case(B, f, T, s):
    """tests/test_gpu_stgcn_kernels.py: test_temporal_conv_forward_fused_bn_relu / test_temporal_conv_gradients"""
    g = torch.Generator().manual_seed(11 * f + T + s)
    x = torch.randn(B, f, T, 25, generator=g).double()
    sc, sh = (1 + 0.2 * torch.randn(f, generator=g)).double(), (0.3 * torch.randn(f, generator=g)).double()
    kernel = (torch.randn(9, 1, f, f, generator=g) * 0.05).double().requires_grad_(True)
    bias = (torch.randn(f, generator=g) * 0.1).double().requires_grad_(True)
    pre = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    y = O.temporal_conv(torch.relu(pre), kernel, bias, s)
    To, pad, _ = O.same_pad(T, 9, s)
    du = torch.randn(B, f, To, 25, generator=g)
    g_pre, g_k, g_b = torch.autograd.grad(y, (pre, kernel, bias), du.double())
    return dict(x=x, sc=sc.float(), sh=sh.float(), kernel=kernel.detach(), bias=bias.detach(), y=y.detach(), To=To, pad=pad, du=du,
                g_pre=g_pre, g_k=g_k, g_b=g_b)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", [(2, 64, 13, 1), (3, 64, 14, 2)])
def test_temporal_conv_forward_fused_prologue_and_stats(dev, B, f, T, s, pad):
    from sar_amd import ops, _lib as L
    c = temporal_case(B, f, T, s)
    To = c["To"]
    W, bias, pro = c["kernel"].float().to(dev), c["bias"].float().to(dev), (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g):
        out = g.out("out", f, B * To * 25)
        r = ops.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), out, W, f * f, f, B=B, V=25, T_src=T, T_out=To, Kc=f, M=f, taps=9,
                          stride=s, pad=c["pad"], bias=bias, pro=pro, pro_relu=True, epi=L.SAR_EPI_STATS)
        g.part("stats", r[0])
        g.ref("temporal forward", out, to_cn(c["y"]), TOL)
        g.ref("sum", lambda: r[0].double().sum(dim=1)[:, 0], c["y"].sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum of squares", lambda: r[0].double().sum(dim=1)[:, 1], (c["y"] * c["y"]).sum(dim=(0, 2, 3)), TOL)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
def test_temporal_conv_data_gradient_masked(dev, pad):
    from sar_amd import ops, _lib as L
    B, f, T, s = 2, 64, 11, 2
    c = temporal_case(B, f, T, s)
    To = c["To"]
    wT = _transposed(dev, c["kernel"], 9, f, f)
    aff = (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g):
        dz = g.out("dz", f, B * T * 25)
        pm = ops.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["du"])), dz, wT, f * f, f, B=B, V=25, T_src=To, T_out=T, Kc=f, M=f, taps=9,
                           stride=s, pad=c["pad"], transposed=True, epi=L.SAR_EPI_MASK, aux=g.inp(to_cn(c["x"])), aux_affine=aff)
        g.part("mask", pm[0])
        g.ref("temporal data gradient", dz, to_cn(c["g_pre"]), TOL)
        g.ref("sum dz", lambda: pm[0].double().sum(dim=1)[:, 0], c["g_pre"].sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum dz x", lambda: pm[0].double().sum(dim=1)[:, 1], (c["g_pre"] * c["x"]).sum(dim=(0, 2, 3)), 1e-4)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", [(2, 64, 13, 1), (3, 64, 14, 2), (2, 64, 11, 2)])
def test_temporal_weight_gradient(dev, B, f, T, s, pad):
    from sar_amd import ops, _lib as L
    c = temporal_case(B, f, T, s)
    pro = (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g):
        flat = g.flat("dW | dbias", 9 * f * f + f)
        ops.conv_wgrad(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), g.inp(to_cn(c["du"])), flat, B=B, V=25, T_src=T, T_out=c["To"], Kc=f, M=f,
                       taps=9, stride=s, pad=c["pad"], pro=pro, pro_relu=True, w_stride_tap=f * f, w_stride_c=f, wsize=9 * f * f, bsize=f)
        g.ref("temporal dW", lambda: flat[:9 * f * f].cpu().view(9, 1, f, f), c["g_k"], TOL)
        g.ref("temporal dbias", lambda: flat[9 * f * f:], c["g_b"], TOL)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ conv_gemm / conv_wgrad: residual 1x1
@functools.lru_cache(maxsize=None)
def residual_case(B, cin, f, T, s):
    """tests/test_gpu_stgcn_kernels.py: test_residual_conv_forward / test_residual_conv_gradients"""
    g = torch.Generator().manual_seed(cin * 3 + f)
    x = torch.randn(B, cin, T, 25, generator=g).double().requires_grad_(True)
    kernel = (torch.randn(1, 1, cin, f, generator=g) * 0.1).double().requires_grad_(True)
    bias = (torch.randn(f, generator=g) * 0.1).double().requires_grad_(True)
    y = F.conv2d(x, O.hwio_to_oihw(kernel), bias, stride=(s, 1))
    dr = torch.randn(B, f, y.shape[2], 25, generator=g)
    gx, gk, gb = torch.autograd.grad(y, (x, kernel, bias), dr.double())
    return dict(x=x.detach(), kernel=kernel.detach(), bias=bias.detach(), y=y.detach(), To=y.shape[2], dr=dr, gx=gx, gk=gk, gb=gb)


@pytest.mark.parametrize("pad", PADS)
def test_residual_conv_forward_data_and_weight_gradient(dev, pad):
    from sar_amd import ops, _lib as L
    B, cin, f, T, s = 2, 64, 128, 13, 2
    c = residual_case(B, cin, f, T, s)
    To = c["To"]
    W, bias = c["kernel"].float().to(dev), c["bias"].float().to(dev)
    rT = _transposed(dev, c["kernel"], 1, cin, f).view(f, cin)

    def fn(g):
        out, dx, flat = g.out("out", f, B * To * 25), g.out("dx", cin, B * T * 25), g.flat("dW | dbias", cin * f + f)
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), out, W, 0, f, B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s,
                      pad=0, bias=bias)
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["dr"])), dx, rT, 0, cin, B=B, V=25, T_src=To, T_out=T, Kc=f, M=cin, taps=1,
                      stride=s, pad=0, transposed=True)
        ops.conv_wgrad(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), g.inp(to_cn(c["dr"])), flat, B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f,
                       taps=1, stride=s, pad=0, w_stride_tap=0, w_stride_c=f, wsize=cin * f, bsize=f)
        g.ref("residual forward", out, to_cn(c["y"]), TOL)
        g.ref("residual data gradient", dx, to_cn(c["gx"]), TOL)
        g.ref("residual dW", lambda: flat[:cin * f].cpu().view(1, 1, cin, f), c["gk"], TOL)
        g.ref("residual dbias", lambda: flat[cin * f:], c["gb"], TOL)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ block tail
TAIL_SHAPES = [(64, 2 * 7 * 25), (20, 776)]


@functools.lru_cache(maxsize=None)
def tail_case(C, n):
    g = torch.Generator().manual_seed(3 * C + n)
    rnd = lambda *s: torch.randn(*s, generator=g)
    u, r, dy = rnd(C, n), rnd(C, n), rnd(C, n)
    sc, sh, rsc, rsh, mu, mr = 1 + 0.2 * rnd(C), 0.3 * rnd(C), 1 + 0.2 * rnd(C), 0.3 * rnd(C), 0.1 * rnd(C), 0.1 * rnd(C)
    k = [rnd(C) for _ in range(6)]
    col = lambda v: v.double().view(-1, 1)
    y = {1: torch.relu(u.double() * col(sc) + col(sh) + r.double()),
         2: torch.relu(u.double() * col(sc) + col(sh) + r.double() * col(rsc) + col(rsh))}
    return dict(u=u, r=r, dy=dy, sc=sc, sh=sh, rsc=rsc, rsh=rsh, mu=mu, mr=mr, k=k, y=y, col=col)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_forward(dev, C, n, kind, pad):
    """sar_bn_add_relu_fwd_f32 without and with a mask: y = relu(u sc + sh + residual).  The mask exists only for rows of 4-element groups
    (ops.relu_mask: n % 4 == 0 and ld % 4 == 0), else relu_mask returns None and the masked kernel rejects the rows."""
    from sar_amd import ops
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    rs = (d(c["rsc"]), d(c["rsh"])) if kind == 2 else (None, None)

    def fn(g):
        u, r, y0 = g.inp(c["u"]), g.inp(c["r"]), g.out("y", C, n)
        ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), kind, r, rs[0], rs[1], y0)
        g.ref("block tail forward", y0, c["y"][kind], TOL)
        m = ops.relu_mask(y0)
        assert (m is None) == bool(n % 4 or (n + g.pad) % 4)
        if m is None:      # the ABI rejects what relu_mask declines, and launches nothing
            y1, whole1 = guarded((C, n), g.pad, SENTINEL, dev, FRONT, BACK)
            with pytest.raises(ops.L.SarError):
                ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), kind, r, rs[0], rs[1], y1,
                                    mask=torch.empty((C, (n + g.pad + 3) // 4), dtype=torch.uint8, device=dev))
            g.ref("the rejected masked call wrote nothing", lambda: (whole1 == SENTINEL).all().reshape(1), torch.ones(1, dtype=torch.bool), 0)
            return
        y1 = g.out("y (masked kernel)", C, n)
        assert tuple(m.shape) == (C, (n + g.pad) // 4)
        mask = g.mask("relu", C, n)
        ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), kind, r, rs[0], rs[1], y1, mask=mask)
        g.ref("masked kernel == plain kernel", y1, y0, 0)
        g.ref("mask == its definition", lambda: mask[:, :n // 4], lambda: mask_bytes(y0 > 0), 0)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_backward_reduce(dev, C, n, pad):
    """sar_bn_add_relu_bwd_reduce_f32, plain, with a mask and with a tail: partials (sum dz, sum dz (u - mu), sum dz (r - mr)), dz = dy where y > 0"""
    from sar_amd import ops
    from sar_amd.stgcn import _BN
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    yv = c["y"][2].float()
    dz = c["dy"].double() * (yv > 0)
    sums = [dz.sum(1), (dz * (c["u"].double() - c["col"](c["mu"]))).sum(1), (dz * (c["r"].double() - c["col"](c["mr"]))).sum(1)]
    gam, rgam = 1 + 0.2 * torch.sin(torch.arange(C, dtype=torch.float32)), 1 + 0.2 * torch.cos(torch.arange(C, dtype=torch.float32))
    rstd = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(C))

    def fn(g):
        dy, y, u, r = g.inp(c["dy"]), g.inp(yv), g.inp(c["u"]), g.inp(c["r"])
        p0, n0 = ops.bn_add_relu_bwd_reduce(dy, y, u, r, d(c["mu"]), d(c["mr"]))
        g.part("plain", p0, 3)
        for j, name in enumerate(("sum dz", "sum dz (u - mu)", "sum dz (r - mr)")):
            g.ref(name, lambda j=j: p0.double().sum(dim=1)[:, j], sums[j], 1e-4)
        if n % 4 == 0 and (n + g.pad) % 4 == 0:
            p1, n1 = ops.bn_add_relu_bwd_reduce(dy, None, u, r, d(c["mu"]), d(c["mr"]), mask=g.mask("relu", C, n, yv > 0))
            assert n1 == n0
            g.part("masked", p1, 3)
            g.ref("masked partials == plain partials", lambda: p1[:, :, :3], lambda: p0[:, :, :3], 0)
        elif n % 4 == 0:
            with pytest.raises(ops.L.SarError):
                ops.bn_add_relu_bwd_reduce(dy, None, u, r, d(c["mu"]), d(c["mr"]), mask=torch.zeros((C, (n + g.pad) // 4 + 1), dtype=torch.uint8, device=dev))
        # the folded finalisation against the separate launches on the plain partials (test_folded_bn_backward_finalisation: 1e-6)
        z = lambda: torch.zeros(C, device=dev)
        gamd, rgamd = d(gam), d(rgam)      # (sar_bn_tail holds raw pointers: the tensors must outlive the launch)
        bn, rbn, bn0, rbn0 = _BN(C, dev), _BN(C, dev), _BN(C, dev), _BN(C, dev)
        for b in (bn, rbn, bn0, rbn0):
            b.rstd.copy_(d(rstd))
        dg0, db0, rdg0, rdb0, dg, db, rdg, rdb = z(), z(), z(), z(), z(), z(), z(), z()
        ops.bn_bwd_finalize(p0, n0, n0 * 4, 4, 0, 1, C, n, gamd, d(c["mu"]), bn0.rstd, dg0, db0, bn0.k1, bn0.k2, bn0.k3)
        ops.bn_bwd_finalize(p0, n0, n0 * 4, 4, 0, 2, C, n, rgamd, d(c["mr"]), rbn0.rstd, rdg0, rdb0, rbn0.k1, rbn0.k2, rbn0.k3)
        tail = ops.make_bn_tail(dev, n, gamd, bn, dg, db, rgamd, rbn, rdg, rdb)
        p2, _ = ops.bn_add_relu_bwd_reduce(dy, y, u, r, d(c["mu"]), d(c["mr"]), tail=tail)
        g.part("tail", p2, 3)
        for name, got, want in [("dgamma", dg, dg0), ("dbeta", db, db0), ("k1", bn.k1, bn0.k1), ("k2", bn.k2, bn0.k2), ("k3", bn.k3, bn0.k3),
                                ("rdgamma", rdg, rdg0), ("rdbeta", rdb, rdb0), ("rk1", rbn.k1, rbn0.k1), ("rk2", rbn.k2, rbn0.k2),
                                ("rk3", rbn.k3, rbn0.k3)]:
            g.part("tail " + name, got)
            g.ref("folded finalisation " + name, got, want, 1e-6)
        g.keep = (gamd, rgamd, bn, rbn)
        g.ref("ticket array back to zero", lambda: ops.bn_tail_tickets(dev).abs().sum().reshape(1).float(), torch.zeros(1), 0)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_backward_apply_and_affine2(dev, C, n, pad):
    """sar_bn_add_relu_bwd_apply_f32 without / with a mask: du = k1 dz + k2 u + k3, dr = rk1 dz + rk2 r + rk3, dz_out = dz; sar_affine2_f32:
    out = k1 a + k2 b + k3 (1e-6: one fused multiply-add chain per element, test_gpu_stgin.py's bar for such kernels)"""
    from sar_amd import ops
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    yv = c["y"][2].float()
    dz = c["dy"].double() * (yv > 0)
    k = [c["col"](v) for v in c["k"]]
    kd = [d(v) for v in c["k"]]

    def fn(g):
        dy, y, u, r = g.inp(c["dy"]), g.inp(yv), g.inp(c["u"]), g.inp(c["r"])
        du, dr, dzo, aff = g.out("du", C, n), g.out("dr", C, n), g.out("dz", C, n), g.out("affine2", C, n)
        ops.bn_add_relu_bwd_apply(dy, y, u, r, kd[:3], kd[3:], du, dr, dzo)
        ops.affine2(u, r, kd[:3], aff)
        g.ref("du", du, k[0] * dz + k[1] * c["u"].double() + k[2], 1e-6)
        g.ref("dr", dr, k[3] * dz + k[4] * c["r"].double() + k[5], 1e-6)
        g.ref("dz_out", dzo, dz, 1e-7)
        g.ref("affine2", aff, k[0] * c["u"].double() + k[1] * c["r"].double() + k[2], 1e-6)
        if n % 4 == 0 and (n + g.pad) % 4 == 0:
            du1, dr1, dz1 = g.out("du (mask)", C, n), g.out("dr (mask)", C, n), g.out("dz (mask)", C, n)
            ops.bn_add_relu_bwd_apply(dy, None, u, r, kd[:3], kd[3:], du1, dr1, dz1, mask=g.mask("relu", C, n, yv > 0))
            for a, b, name in ((du1, du, "du"), (dr1, dr, "dr"), (dz1, dzo, "dz")):
                g.ref("masked %s == plain" % name, a, b, 0)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ data_bn, pool, transpose
@functools.lru_cache(maxsize=None)
def data_bn_case():
    """tests/test_gpu_stgcn_kernels.py: test_data_bn_forward_backward (N, T = 3, 17)"""
    p = O.randomize_affine(O.init_params(5, blocks=[(64, 1, False)]))
    x, _ = O.synthetic_batch(3, seed=4, T=17, num_classes=5)
    pd = {k: v.double() for k, v in p.items()}
    gam, bet = pd["data_bn.gamma"].clone().requires_grad_(True), pd["data_bn.beta"].clone().requires_grad_(True)
    pd["data_bn.gamma"], pd["data_bn.beta"] = gam, bet
    ref = O.data_bn(x.double(), pd, True, {})
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(1))
    gg, gb = torch.autograd.grad(ref, (gam, bet), dy.double())
    return p, x, ref.detach(), dy, gg, gb


@pytest.mark.parametrize("pad", PADS)
def test_data_bn_apply_and_backward_reduce(dev, pad):
    from sar_amd import ops
    p, x, ref, dy, gg, gb = data_bn_case()
    N, C, T, V, M = x.shape
    xg = x.to(dev)
    z = lambda: torch.empty(V * C, device=dev)
    part = torch.empty((V * C, N, 2), device=dev)
    mean, rstd, scale, shift = z(), z(), z(), z()
    ops.data_bn_stats(xg, None, part)
    ops.bn_finalize(part, N, V * C, N * M * T, 1e-3, 0.99, False, p["data_bn.gamma"].to(dev), p["data_bn.beta"].to(dev),
                    p["data_bn.moving_mean"].to(dev), p["data_bn.moving_var"].to(dev), mean, rstd, scale, shift)

    def fn(g):
        out = g.out("out", C, N * M * T * V)
        ops.data_bn_apply(xg, None, scale, shift, out)
        g.ref("data_bn forward", out, to_cn(ref), TOL)
        bpart = torch.empty((V * C, N, 2), device=dev)
        ops.data_bn_bwd_reduce(xg, None, g.inp(to_cn(dy)), mean, bpart)
        g.part("backward", bpart)
        dgam, dbet = z(), z()
        ops.bn_bwd_finalize(bpart, N, N * 2, 2, 0, 1, V * C, N * M * T, p["data_bn.gamma"].to(dev), mean, rstd, dgam, dbet)
        g.ref("data_bn dgamma", dgam, gg, TOL)
        g.ref("data_bn dbeta", dbet, gb, TOL)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
def test_pool_forward_and_backward(dev, pad):
    """tests/test_gpu_stgcn_kernels.py: test_head_loss_and_sgd's pooling (C = 256, N Mp = 10, TV = 75)"""
    from sar_amd import ops
    g0 = torch.Generator().manual_seed(9)
    N, Mp, C, TV = 5, 2, 256, 75
    y = torch.randn(C, N * Mp * TV, generator=g0)
    dfeat = torch.randn(N, C, generator=g0)
    feat_ref = y.double().view(C, N * Mp, TV).mean(2).t().reshape(N, Mp, C).mean(1)
    dy_ref = (dfeat.double().t().contiguous() / (Mp * TV)).view(C, N, 1).expand(C, N, Mp * TV).reshape(C, N * Mp * TV)

    def fn(g):
        feat, dy = g.flat("feat", N * C), g.out("dy", C, N * Mp * TV)
        ops.pool_fwd(g.inp(y), N * Mp, TV, Mp, feat.view(N, C))
        ops.pool_bwd(dfeat.to(dev), N * Mp, TV, Mp, dy)
        g.ref("pooled features", lambda: feat.view(N, C), feat_ref, TOL)
        g.ref("pool backward", dy, dy_ref, TOL)
    drive(dev, fn, pad)


def test_transpose_one_batch(dev):
    """sar_transpose_f32 takes no leading dimension: one batch of 25 x 33 between two guarded flat ranges (a pure copy: bitwise)"""
    from sar_amd import ops
    x = torch.randn(25, 33, generator=torch.Generator().manual_seed(2))
    g = Launch(dev, 0)
    src, _ = guarded_flat(x, NAN, dev, KFLAT)
    out = g.flat("out", 25 * 33)
    ops.transpose(src, out, 1, 25, 33)
    g.ref("transpose", lambda: out.view(33, 25), x.t().contiguous(), 0)
    torch.cuda.synchronize()
    g.check()


# ------------------------------------------------------------------------------------------------ dense adjacency (shared / per frame)
DENSE_SHAPES = [(1, 20, 9, 25), (2, 16, 5, 18)]
K = 3


@functools.lru_cache(maxsize=None)
def dense_case(B, Fc, T, V, per_frame):
    """tests/test_gpu_adjacency.py: test_dense_contraction_kernels / tests/test_gpu_stgcn_ta.py: test_contraction_kernels_against_float64"""
    g = torch.Generator().manual_seed(B * 100 + Fc)
    y = torch.randn(B, K * Fc, T, V, generator=g)
    A = torch.randn(*((K, T, V, V) if per_frame else (K, V, V)), generator=g) * 0.3
    dout = torch.randn(B, Fc, T, V, generator=g)
    addv = torch.randn(B, Fc, T, V, generator=g)
    yd, Ad = y.double().view(B, K, Fc, T, V).requires_grad_(True), A.double().requires_grad_(True)
    ref = torch.einsum("nkctv,ktvw->nctw" if per_frame else "nkctv,kvw->nctw", yd, Ad)
    gy, gA = torch.autograd.grad(ref, (yd, Ad), dout.double())
    return y, A, dout, addv, cn(ref.detach()), cn(gy.reshape(B, K * Fc, T, V)), gA


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("per_frame", [False, True], ids=["graph_dense", "graph_dense_t"])
@pytest.mark.parametrize("B,Fc,T,V", DENSE_SHAPES)
def test_dense_adjacency_kernels(dev, B, Fc, T, V, per_frame, pad):
    from sar_amd import ops
    y, A, dout, addv, refc, gyc, gA = dense_case(B, Fc, T, V, per_frame)
    n = B * T * V
    Ac = A.to(dev).contiguous()
    refa = refc + cn(addv).double()

    def fn(g):
        yc, dc = g.inp(cn(y)), g.inp(cn(dout))
        out, out_add, dy, dA = g.out("out", Fc, n), g.out("out + add", Fc, n), g.out("dy", K * Fc, n), g.flat("dA", A.numel())
        if per_frame:
            part, _ = ops.graph_dense_t_fwd(yc, Ac, out, K, Fc, V, B, T, stats=True)
            part_add, _ = ops.graph_dense_t_fwd(yc, Ac, out_add, K, Fc, V, B, T, stats=True, add=g.inp(cn(addv)))
            ops.graph_dense_t_bwd_data(dc, Ac, dy, K, Fc, V, B, T)
            ops.graph_dense_t_dA(yc, dc, dA.view(K, T, V, V), K, Fc, V, B, T)
        else:
            part, _ = ops.graph_dense_fwd(yc, Ac, out, K, Fc, V, B * T, stats=True)
            part_add, _ = ops.graph_dense_fwd(yc, Ac, out_add, K, Fc, V, B * T, stats=True, add=g.inp(cn(addv)))
            ops.graph_dense_bwd_data(dc, Ac, dy, K, Fc, V, B * T)
            ops.graph_dense_dA(yc, dc, dA.view(K, V, V), K, Fc, V, B * T, nsplit=3)
        g.part("stats", part)
        g.part("stats (add)", part_add)
        g.ref("out", out, refc, 2e-5)
        g.ref("sum", lambda: part.double().sum(dim=1)[:, 0], refc.sum(dim=1), 1e-4)
        g.ref("sum of squares", lambda: part.double().sum(dim=1)[:, 1], (refc * refc).sum(dim=1), 2e-5)
        g.ref("out + add", out_add, refa, 2e-5)
        g.ref("sum (add)", lambda: part_add.double().sum(dim=1)[:, 0], refa.sum(dim=1), 1e-4)
        g.ref("sum of squares (add)", lambda: part_add.double().sum(dim=1)[:, 1], (refa * refa).sum(dim=1), 2e-5)
        g.ref("dy", dy, gyc, 2e-5)
        g.ref("dA", lambda: dA.view(A.shape), gA, 2e-5)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ GIN
@pytest.mark.parametrize("pad", PADS)
def test_graph_gather_kernels(dev, pad):
    """tests/test_gpu_stgin.py: test_graph_gather_kernels at (F, frames) = (3, 17)"""
    from sar_amd import ops
    from oracle.graph import spatial_adjacency
    Fc, frames, V = 3, 17, 25
    A_ext = np.concatenate([spatial_adjacency().astype(np.float32)[:2], np.eye(V, dtype=np.float32)[None]])
    tf_, tb_ = ops.GraphTables(A_ext, dev, transpose=False), ops.GraphTables(A_ext, dev, transpose=True)
    g0 = torch.Generator().manual_seed(Fc + frames)
    n = frames * V
    x, dz, add = torch.randn(Fc, n, generator=g0), torch.randn(K * Fc, n, generator=g0), torch.randn(Fc, n, generator=g0)
    sc = torch.tensor([1.0, 1.0, 1.3])
    At = torch.from_numpy(A_ext).double()
    ref_z = torch.einsum("ctv,kvw->kctw", x.double().view(Fc, frames, V), At).reshape(K * Fc, n)
    ref_s = torch.einsum("kctw,kvw->ctv", dz.double().view(K, Fc, frames, V) * sc.double().view(K, 1, 1, 1), At).reshape(Fc, n) + add.double()

    def fn(g):
        z, out = g.out("expand", K * Fc, n), g.out("sum", Fc, n)
        ops.graph_gather_expand(g.inp(x), tf_, K, Fc, V, z)
        ops.graph_gather_sum(g.inp(dz), tb_, sc.to(dev), K, Fc, V, out, add=g.inp(add))
        g.ref("gather expand", z, ref_z, 1e-6)
        g.ref("gather sum", out, ref_s, 1e-6)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def gin_case(C, n):
    """tests/test_gpu_stgin.py: test_gin_elementwise_kernels"""
    g = torch.Generator().manual_seed(C + n)
    a = torch.randn(K * C, n, generator=g)
    sc, sh = 1 + 0.3 * torch.randn(K * C, generator=g), 0.3 * torch.randn(K * C, generator=g)
    mean = 0.2 * torch.randn(K * C, generator=g)
    ds = torch.randn(C, n, generator=g)
    ks = [torch.randn(K * C, generator=g) for _ in range(3)]
    ad = a.double()
    post = torch.relu(ad * sc.double()[:, None] + sh.double()[:, None])
    dz = ds.double().repeat(K, 1) * (post > 0)
    return a, sc, sh, mean, ds, ks, post.view(K, C, n).sum(0), dz


@pytest.mark.parametrize("pad", PADS)
def test_gin_elementwise_kernels(dev, pad):
    """(C, n) = (8, 376): n % 4 == 0, so the two reducing kernels need 16-byte aligned rows (csrc/gin.hip: "with n % 4 == 0 the rows must
    be 16-byte aligned") and reject pad = 7; gin_sum_fwd without statistics and gin_bwd_apply take every ld."""
    from sar_amd import ops
    C, n = 8, 3 * 25 * 5 + 1
    a, sc, sh, mean, ds, ks, s_ref, dz = gin_case(C, n)
    d = lambda t: t.to(dev)
    aligned = (n + pad) % 4 == 0

    def fn(g):
        ag, dsg = g.inp(a), g.inp(ds)
        s, da = g.out("s", C, n), g.out("da", K * C, n)
        if aligned or g.pad == 0:
            part, _ = ops.gin_sum_fwd(ag, d(sc), d(sh), K, s, stats=True)
            g.part("stats", part)
            g.ref("sum", lambda: part.double().sum(1)[:, 0], s_ref.sum(1), 1e-5)
            g.ref("sum of squares", lambda: part.double().sum(1)[:, 1], (s_ref * s_ref).sum(1), 1e-5)
            bpart, _ = ops.gin_bwd_reduce(dsg, ag, d(sc), d(sh), d(mean), K)
            g.part("backward", bpart)
            g.ref("sum dz", lambda: bpart.double().sum(1)[:, 0], dz.sum(1), 1e-5)
            g.ref("sum dz (a - mean)", lambda: bpart.double().sum(1)[:, 1], (dz * (a.double() - mean.double()[:, None])).sum(1), 1e-5)
        else:
            ops.gin_sum_fwd(ag, d(sc), d(sh), K, s)
        ops.gin_bwd_apply(dsg, ag, d(sc), d(sh), tuple(d(k) for k in ks), K, da)
        g.ref("gin sum", s, s_ref, 1e-6)
        g.ref("gin backward apply", da, ks[0].double()[:, None] * dz + ks[1].double()[:, None] * a.double() + ks[2].double()[:, None], 1e-6)
    drive(dev, fn, pad)
    if not aligned:
        rejected(dev, lambda g: ops.gin_sum_fwd(g.inp(a), d(sc), d(sh), K, g.out("s", C, n), stats=True), pad)
        rejected(dev, lambda g: ops.gin_bwd_reduce(g.inp(ds), g.inp(a), d(sc), d(sh), d(mean), K), pad)


# ------------------------------------------------------------------------------------------------ projection graph convolution
@functools.lru_cache(maxsize=None)
def pgc_case(B, T):
    """tests/test_gpu_stpgcn.py: _layer_case / test_layer_against_float64"""
    import pgc_reference as R
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.relu(torch.randn(B, 64, T, 25, generator=g))
    p = R.init_pgc({}, B * 100 + T + 1, dtype=torch.float32)
    prm = [p[k] for k in R.NAMES]
    dout = torch.randn(B, 64, T, 25, generator=g)
    ref, ctx = R.pgc_forward(x.double(), *(t.double() for t in prm))
    grads = R.pgc_backward(ctx, dout.double())
    ref32, ctx32 = R.pgc_forward(x, *prm)
    grads32 = R.pgc_backward(ctx32, dout)
    return x, prm, dout, ref, ctx["q"], grads, grads32


@pytest.mark.parametrize("pad", PADS)
def test_projection_graph_convolution(dev, pad):
    """pgc_forward / pgc_backward at B, T = 3, 17 with x, dout, out and dx padded (operands.cn_matrix: any ld >= B P).  Bars: 1e-4, and for
    the two all-column sums eight times the float32 restatement's own distance from float64 (tests/test_gpu_stpgcn.py: _judge)."""
    from sar_amd import ops
    B, T = 3, 17
    P = T * 25
    x, prm, dout, ref, q_ref, grads, grads32 = pgc_case(B, T)
    cen, var, W, b = (t.contiguous().to(dev) for t in prm)

    def band(i):
        return max(1e-4, 8 * rel_err(grads32[i], grads[i]))

    def fn(g):
        xg, dg = g.inp(to_cn(x)), g.inp(to_cn(dout))
        out, dx = g.out("out", 64, B * P), g.out("dx", 64, B * P)
        gc, gv, gwb = g.flat("g_centers", cen.numel()), g.flat("g_variance", var.numel()), g.flat("g_kernel | g_bias", 64 * 64 + 64)
        q, sv = ops.pgc_forward(xg, B, P, cen, var, W, b, out)
        ops.pgc_backward(xg, dg, q, sv, B, P, cen, var, W, dx, gc.view(cen.shape), gv.view(var.shape), gwb)
        g.part("q", q)
        g.part("saved", sv)
        g.ref("out", out, to_cn(ref), 1e-4)
        g.ref("q", lambda: q.cpu().view(32, B, P).permute(1, 2, 0), q_ref, 1e-4)
        g.ref("dx", dx, to_cn(grads[0]), 1e-4)
        g.ref("pgc.centers", lambda: gc.view(cen.shape), grads[1], band(1))
        g.ref("pgc.variance", lambda: gv.view(var.shape), grads[2], band(2))
        g.ref("pgc.gcn.kernel", lambda: gwb[:4096].cpu().view(1, 64, 64), grads[3], 1e-4)
        g.ref("pgc.gcn.bias", lambda: gwb[4096:], grads[4], 1e-4)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ 2-D convolutions
# (cin, cout, k, stride, H, W): the smallest shapes of tests/test_gpu_conv2d_kernels.py, the stem at H = 32, and two rectangular images
# (every other fp32 2-D test is square: an H / W exchange in the geometry would pass them)
C2D_SHAPES = [(8, 8, 3, 1, 16, 16), (24, 40, 3, 1, 20, 20), (16, 32, 3, 2, 64, 64), (1, 64, 7, 2, 32, 32), (8, 8, 3, 1, 12, 20),
              (16, 32, 3, 2, 12, 20),
              # one case each of groups B, C and F of tests/conv2d_rect_cases.py: 1x1 / stride 2 onto 7 x 9, the stem at 25 x 35, the
              # fixed-geometry weight gradient v3 with a ragged last row tile (H_out = 11, th = 8)
              (8, 16, 1, 2, 13, 18), (1, 40, 7, 2, 25, 35), (24, 40, 3, 1, 11, 16)]


@functools.lru_cache(maxsize=None)
def conv2d_case(cin, cout, k, s, H, Wd, B=2):
    """tests/test_gpu_conv2d_kernels.py: test_conv2d_forward_dgrad_wgrad, against torch.nn.functional.conv2d in float64"""
    pad, taps = k // 2, k * k
    g = torch.Generator().manual_seed(cin * 7 + cout + k + s)
    x = torch.randn(B, cin, H, Wd, generator=g).double().requires_grad_(True)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * taps) ** 0.5).double().requires_grad_(True)
    sc, sh = (1 + 0.2 * torch.randn(cin, generator=g)).double(), (0.3 * torch.randn(cin, generator=g)).double()
    use_pro = cin > 1
    hin = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if use_pro else x
    y = F.conv2d(hin, w, None, stride=s, padding=pad)
    dy = torch.randn(y.shape, generator=g)
    gh, gw = torch.autograd.grad(y, (hin, w), dy.double())
    add = torch.randn(cin, B * H * Wd, generator=g)
    return dict(x=x.detach(), w=w.detach(), sc=sc.float(), sh=sh.float(), use_pro=use_pro, y=y.detach(), dy=dy, gh=gh, gw=gw, add=add,
                Ho=y.shape[2], Wo=y.shape[3])


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("cin,cout,k,s,H,Wd", C2D_SHAPES)
def test_conv2d_forward_data_and_weight_gradient(dev, cin, cout, k, s, H, Wd, pad):
    from sar_amd import ops, _lib as L
    B, taps = 2, k * k
    c = conv2d_case(cin, cout, k, s, H, Wd)
    Ho, Wo = c["Ho"], c["Wo"]
    geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=Wd, H_out=Ho, W_out=Wo, KH=k, KW=k, stride=s, pad=k // 2)
    wd = c["w"].float().to(dev).contiguous()
    wf, wb = torch.empty(taps * cin * cout, device=dev), torch.empty(taps * cin * cout, device=dev)
    ops.permute3(wd, wf, taps, cin, cout, 1, taps, cin * taps)
    ops.permute3(wd, wb, taps, cout, cin, 1, cin * taps, taps)
    pro = (c["sc"].to(dev), c["sh"].to(dev)) if c["use_pro"] else None

    def fn(g):
        xd, dyd = g.inp(cn(c["x"])), g.inp(cn(c["dy"]))
        out, dW = g.out("out", cout, B * Ho * Wo), g.flat("dW", taps * cin * cout)
        r = ops.conv2d_gemm(xd, out, wf, cin * cout, cout, epi=L.SAR_EPI_STATS, pro=pro, pro_relu=c["use_pro"], **geo)
        g.part("stats", r[0])
        g.ref("conv2d forward", out, cn(c["y"]), TOL)
        g.ref("sum of squares", lambda: r[0].double().sum(1)[:, 1], (c["y"] * c["y"]).sum(dim=(0, 2, 3)), TOL)
        ops.conv2d_wgrad(xd, dyd, dW, pro=pro, pro_relu=c["use_pro"], **geo)
        gwd = torch.empty((cout, cin, k, k), device=dev)
        g.ref("conv2d weight gradient", lambda: (ops.permute3(dW.contiguous(), gwd, cout, cin, taps, 1, cout, cin * cout), gwd)[1], c["gw"], TOL)
        if cin > 1:      # (no data gradient for the 1-channel stem)
            dx = g.out("dx", cin, B * H * Wd)
            ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(c["add"]), B=B, Kc=cout, M=cin, H_src=Ho, W_src=Wo,
                            H_out=H, W_out=Wd, KH=k, KW=k, stride=s, pad=k // 2, transposed=True)
            g.ref("conv2d data gradient", lambda: dx.cpu() - c["add"], cn(c["gh"]), TOL)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def parity_case(cin, cout, H, B=3):
    """tests/test_gpu_conv2d_kernels.py: test_stride2_data_gradient_parity_classes"""
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(B, cin, H, H, generator=g).double().requires_grad_(True)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).double()
    y = F.conv2d(x, w, None, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g)
    gx, = torch.autograd.grad(y, x, dy.double())
    aux = torch.randn(cin, B * H * H, generator=g)
    sc, sh, mu = 1 + 0.2 * torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    small = torch.randn(cin, B * y.shape[2] * y.shape[2], generator=g)
    return w, dy, gx, aux, sc, sh, mu, small, y.shape[2]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("cin,cout,H", [(8, 16, 15), (16, 32, 12)])
def test_conv2d_stride2_data_gradient_parity_classes(dev, cin, cout, H, pad):
    """the MASK epilogue with its partial sums over the four parity-class launches, and (H even) the compact aux at the even pixels"""
    from sar_amd import ops, _lib as L
    B = 3
    w, dy, gx, aux, sc, sh, mu, small, Ho = parity_case(cin, cout, H)
    wb = torch.empty(9 * cin * cout, device=dev)
    ops.permute3(w.float().to(dev).contiguous(), wb, 9, cout, cin, 1, cin * 9, 9)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Ho, H_out=H, W_out=H, KH=3, KW=3, stride=2, pad=1, transposed=True)
    ref = cn(gx) * ((aux.double() * sc.double()[:, None] + sh.double()[:, None]) > 0)
    full = torch.zeros(B, cin, H, H, dtype=torch.float64)
    if H % 2 == 0:
        full[:, :, ::2, ::2] = small.double().reshape(cin, B, Ho, Ho).permute(1, 0, 2, 3)

    def fn(g):
        dyd = g.inp(cn(dy))
        dx = g.out("dx", cin, B * H * H)
        r = ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=g.inp(aux), aux_affine=(sc.to(dev), sh.to(dev)),
                            aux_mean=mu.to(dev), **geo)
        g.part("mask", r[0])
        g.ref("masked data gradient", dx, ref, TOL)
        g.ref("sum dz", lambda: r[0].double().sum(1)[:, 0], ref.sum(1), 1e-4)
        g.ref("sum dz (aux - mean)", lambda: r[0].double().sum(1)[:, 1], (ref * (aux.double() - mu.double()[:, None])).sum(1), 1e-4)
        if H % 2 == 0:
            dx2 = g.out("dx + even pixels", cin, B * H * H)
            ops.conv2d_gemm(dyd, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(small), aux_even_pixels=True, **geo)
            g.ref("data gradient + compact aux", dx2, cn(gx + full), TOL)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("cin,cout,H,W", RC.A_PARITY + RC.A_MASKED)
def test_conv2d_stride2_data_gradient_rectangular(dev, cin, cout, H, W, pad):
    """group A of tests/conv2d_rect_cases.py: H x W images, both sides even (parity classes, with the compact aux) or not (masked kernel)"""
    from sar_amd import ops, _lib as L
    B = RC.A_BATCH
    c = RC.conv_ref(cin, cout, 3, 2, H, W, B)
    Ho, Wo = c["Ho"], c["Wo"]
    wb = c["w"].permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)          # (tap, m, c)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Wo, H_out=H, W_out=W, KH=3, KW=3, stride=2, pad=1, transposed=True)

    def fn(g):
        dyd = g.inp(cn(c["dy"]))
        dx = g.out("dx", cin, B * H * W)
        r = ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=g.inp(c["aux"]),
                            aux_affine=(c["sc2"].to(dev), c["sh2"].to(dev)), aux_mean=c["mu"].to(dev), **geo)
        g.part("mask", r[0])
        g.ref("masked data gradient", dx, c["dz"], TOL)
        g.ref("sum dz", lambda: r[0].double().sum(1)[:, 0], c["dz_sum"], 1e-4)
        g.ref("sum dz (aux - mean)", lambda: r[0].double().sum(1)[:, 1], c["dz_cen"], 1e-4)
        if RC.dgrad_s2_route(H, W) == "parity":
            dx2 = g.out("dx + even pixels", cin, B * H * W)
            ops.conv2d_gemm(dyd, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(c["small"]), aux_even_pixels=True, **geo)
            g.ref("data gradient + compact aux", dx2, cn(c["gh_even"]), TOL)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def maxpool_case():
    """tests/test_gpu_conv2d_kernels.py: test_stem_tail_maxpool_forward_backward"""
    g = torch.Generator().manual_seed(3)
    B, C, H = 2, 8, 30
    x = torch.randn(B, C, H, H, generator=g).double().requires_grad_(True)
    sc, sh = (1 + 0.2 * torch.randn(C, generator=g)).double(), (0.3 * torch.randn(C, generator=g)).double()
    y = F.max_pool2d(torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), 3, 2, 1)
    dy = torch.randn(y.shape, generator=g)
    (gx,) = torch.autograd.grad(y, x, dy.double())
    return x.detach(), sc, sh, y.detach(), dy, gx / sc.view(1, -1, 1, 1)


@pytest.mark.parametrize("pad", PADS)
def test_bn_relu_maxpool_forward_and_backward(dev, pad):
    from sar_amd import ops
    B, C, H = 2, 8, 30
    x, sc, sh, y, dy, gz = maxpool_case()
    Ho = y.shape[2]
    scd, shd = sc.float().to(dev), sh.float().to(dev)
    mean64 = x.mean(dim=(0, 2, 3))

    def fn(g):
        xd = g.inp(cn(x))
        yd, dz = g.out("y", C, B * Ho * Ho), g.out("dz", C, B * H * H)
        ops.bn_relu_maxpool_fwd(xd, scd, shd, yd, B, H, H)
        part, _ = ops.bn_relu_maxpool_bwd(xd, scd, shd, mean64.float().to(dev), g.inp(cn(dy)), dz, B, H, H)
        g.part("backward", part)
        g.ref("max-pool forward", yd, cn(y), TOL)
        g.ref("max-pool backward", dz, cn(gz), TOL)
        g.ref("sum dz", lambda: part.double().sum(1)[:, 0], gz.sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum dz (x - mean)", lambda: part.double().sum(1)[:, 1], (gz * (x - mean64.view(1, -1, 1, 1))).sum(dim=(0, 2, 3)), 1e-4)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,C,H,W", RC.E_CASES)
def test_bn_relu_maxpool_forward_and_backward_rectangular(dev, B, C, H, W, pad):
    """group E of tests/conv2d_rect_cases.py: H x W images; (18, 131) and (17, 260) tile the backward 2 x 2 and 2 x 3"""
    from sar_amd import ops
    c = RC.maxpool_ref(B, C, H, W)
    Ho, Wo = c["Ho"], c["Wo"]
    scd, shd = c["sc"].to(dev), c["sh"].to(dev)

    def fn(g):
        xd = g.inp(cn(c["x"]))
        yd, dz = g.out("y", C, B * Ho * Wo), g.out("dz", C, B * H * W)
        ops.bn_relu_maxpool_fwd(xd, scd, shd, yd, B, H, W)
        part, _ = ops.bn_relu_maxpool_bwd(xd, scd, shd, c["mean"].float().to(dev), g.inp(cn(c["dy"])), dz, B, H, W)
        g.part("backward", part)
        g.ref("max-pool forward", yd, cn(c["y"]), TOL)
        g.ref("max-pool backward", dz, cn(c["gz"]), TOL)
        g.ref("sum dz", lambda: part.double().sum(1)[:, 0], c["gz_sum"], 1e-4)
        g.ref("sum dz (x - mean)", lambda: part.double().sum(1)[:, 1], c["gz_cen"], 1e-4)
    drive(dev, fn, pad)
