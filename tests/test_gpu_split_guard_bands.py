"""Guard bands for the split-arithmetic kernels and the bound cells behind the C ABI ("The leading-dimension contract";
csrc/conv_gemm_split.hip, conv_wgrad_split.hip, conv2d_split.hip, conv2d_wgrad_split*.hip and the bound producers of
csrc/elementwise.hip), in the form of tests/test_gpu_guard_bands.py: every operand is a view into a larger allocation -- ld = n + pad
columns per row, 4 rows in front and 16 behind an input (a stager that rounds Kc up to its group of 8 / 16 channels lands in NaN
of the same allocation), 4 / 2 around an output -- whose every other element holds a known fill: NaN around inputs, -7.25 around
outputs, 0xA5 around mask bytes.  Each kernel runs tight (pad = 0), with pad = 4 and with pad = 7, in both arithmetics of the
engines ("f16x3a", "bf16x6"), `split=` given on every call; after each launch

  1. the live region meets the float64 bar of the kernel's own test in tests/test_gpu_split.py (TOL = 2e-5 norm-wise on the same
     oracle functions, the sums at the tolerances stated there and in tests/test_gpu_guard_bands.py for the shared epilogues);
  2. the live region is bitwise the tight launch's (a kernel that picks another summation order for a padded ld says so below);
  3. every guard element of every output still holds its fill, bit for bit;
  4. every output and every reduction partial is finite: no NaN of an input's padding reached a result;
  5. where the ABI rejects the leading dimension, the call raises (or relu_mask returns None) and the outputs hold only the fill.

Particular to this family:
  * ops falls back to the fp32 kernels silently, so every launch is preceded by the project's own query that the split kernel
    takes it (ops.split_applicable, ops.conv2d_split_applicable, sar_conv_wgrad_split_blocks > 0, sar_conv2d_wgrad_split_blocks > 0);
  * the f16x3a operand scale comes from bound cells that ops._src_bound_single raises from the PADDED view: one NaN read from a row's
    padding makes every output of the launch NaN and fails 4;
  * every weight gradient writes its slabs into a NaN-prefilled guarded range (util.GuardedSlabs): an element no workgroup wrote
    reaches dW as NaN and fails 4, a write past nsplit * (wsize + bsize) fails 3;
  * 5 is ld = n - 1 for each of ld_src, ld_out, ld_aux, ld_dout (ld_aux2: n - 4, a multiple of 4 below n).

The guards are part of the operand's own allocation, so a stray access shows as a failed assertion, never as a fault.

Rectangular 2-D cases (tests/conv2d_rect_cases.py): the two smallest cases of group A on conv2d_split_dgrad_s2_kernel and the four
cases of group F that sar_conv2d_wgrad_split_blocks accepts (widths 64, 32, 16, 8 at heights 5, 6, 11, 7).  Worst error over the 2-D
cases of this file in both arithmetics, MEASURED on an MI355X: A masked data gradient 3.1e-7, its sums 5.7e-7 / 7.5e-7, with the
compact aux 2.6e-7; F weight gradient 3.2e-7."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv2d_rect_cases as RC
from oracle import stgcn as O
from test_gpu_guard_bands import TAIL_SHAPES, _A, _tables, _transposed, cn, parity_case, tail_case
from util import MASK_FILL, NAN, SENTINEL, Launch, assert_flat_guards_untouched, drive, guarded, guarded_flat, rejected, to_cn

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # tests/test_gpu_split.py
ARITHS = ["f16x3a", "bf16x6"]
PADS = [4, 7]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class SplitLaunch(Launch):
    IN_BACK = 16      # a channel group of 8 / 16 rounded up from the last live row stays inside the allocation, in NaN


def _drive(dev, fn, pad, bitwise=True):
    return drive(dev, fn, pad, bitwise, launch=SplitLaunch)


def _rejected(dev, fn, short):
    """5: the operand `short` has ld = n - 1 (tight rows of n - 1 columns under a live width of n)"""
    rejected(dev, lambda g: fn(g, short), 0, launch=SplitLaunch)


def _cut(short):
    return lambda name, n: (n - (4 if name == "ld_aux2" else 1)) if short == name else n


def _slab_reduce(slab, nsplit, n, out):
    from sar_amd import _lib as L
    L.check(L.load().sar_slab_reduce_f32(L.ptr(slab), nsplit, slab.stride(0), n, L.ptr(out), L.stream_ptr()), "sar_slab_reduce_f32")


def _bits(x):
    return np.float32(x).view(np.uint32).item()


def _cell_bits(cell):
    return cell.item() & 0xffffffff


def _wgrad_blocks(arith, mode, src, dout, *, B, T_src, T_out, Kc, M, taps, stride=1, pad=0, pro=None, tables=None):
    """sar_conv_wgrad_split_blocks of the descriptor ops.conv_wgrad builds: (blocks, wk, tile positions)"""
    import ctypes as C
    from sar_amd import _lib as L
    d = L.WgradDesc()
    d.mode, d.B, d.V, d.T_src, d.T_out, d.Kc, d.M = mode, B, 25, T_src, T_out, Kc, M
    d.taps, d.stride, d.pad = taps, stride, pad
    d.src, d.ld_src, d.dout, d.ld_dout = L.ptr(src), src.stride(0), L.ptr(dout), dout.stride(0)
    if pro is not None:
        d.pro_scale, d.pro_shift = L.ptr(pro[0]), L.ptr(pro[1])
    if tables is not None:
        d.g_idx, d.g_wt, d.g_colsum = L.ptr(tables.idx), L.ptr(tables.wt), L.ptr(tables.colsum)
        for i in range(3):
            d.nz[i] = tables.nz[i]
        d.g_flags = tables.g_flags
    wk, kt = C.c_int(0), C.c_int(0)
    return L.load().sar_conv_wgrad_split_blocks(C.byref(d), L.SAR_SPLIT[arith], C.byref(wk), C.byref(kt)), wk.value, kt.value


# ------------------------------------------------------------------------------------------------ sar_conv_gemm_split / _wgrad_split: 9 taps
@functools.lru_cache(maxsize=None)
def temporal_case(B, cin, f, T, s):
    """Conv2D(f, [9, 1], strides [s, 1], 'same') behind a folded BatchNorm + ReLU, and its gradients, in float64: computed once"""
    g = torch.Generator().manual_seed(11 * f + 3 * cin + T + s)
    x = torch.randn(B, cin, T, 25, generator=g).double()
    sc, sh = (1 + 0.2 * torch.randn(cin, generator=g)).double(), (0.3 * torch.randn(cin, generator=g)).double()
    kernel = (torch.randn(9, 1, cin, f, generator=g) * 0.05).double().requires_grad_(True)
    bias = (torch.randn(f, generator=g) * 0.1).double().requires_grad_(True)
    pre = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    y = O.temporal_conv(torch.relu(pre), kernel, bias, s)
    To, pad, _ = O.same_pad(T, 9, s)
    du = torch.randn(B, f, To, 25, generator=g)
    g_pre, g_k, g_b = torch.autograd.grad(y, (pre, kernel, bias), du.double())
    return dict(x=x, sc=sc.float(), sh=sh.float(), kernel=kernel.detach(), bias=bias.detach(), y=y.detach(), To=To, pad=pad, du=du,
                g_pre=g_pre, g_k=g_k, g_b=g_b)


def temporal_forward(dev, arith, B, cin, f, T, s):
    """conv_gemm_split_kernel<0, AR, 0 / 1>: forward with the folded BatchNorm + ReLU prologue and the STATS epilogue"""
    from sar_amd import ops, _lib as L
    c = temporal_case(B, cin, f, T, s)
    To, n, no = c["To"], B * T * 25, B * c["To"] * 25
    W, bias, pro = c["kernel"].float().to(dev), c["bias"].float().to(dev), (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g, short=None):
        cut = _cut(short)
        src, out = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.out("out", f, cut("ld_out", no))
        assert ops.split_applicable(L.SAR_CONV_TEMPORAL, 25, cin, f, 9, s, None, pro, False, c["pad"])
        r = ops.conv_gemm(L.SAR_CONV_TEMPORAL, src, out, W, cin * f, f, B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=9, stride=s,
                          pad=c["pad"], bias=bias, pro=pro, pro_relu=True, epi=L.SAR_EPI_STATS, split=arith)
        g.part("stats", r[0])
        g.ref("temporal forward", out, to_cn(c["y"]), TOL)
        g.ref("sum", lambda: r[0].double().sum(dim=1)[:, 0], c["y"].sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum of squares", lambda: r[0].double().sum(dim=1)[:, 1], (c["y"] * c["y"]).sum(dim=(0, 2, 3)), TOL)
    return fn


def temporal_data_gradient(dev, arith, B, cin, f, T, s):
    """conv_gemm_split_kernel<1 / 3, AR, 0>: the data gradient (Kc = f, M = cin) with the MASK epilogue and its sums"""
    from sar_amd import ops, _lib as L
    c = temporal_case(B, cin, f, T, s)
    To, n, no = c["To"], B * T * 25, B * c["To"] * 25
    wT = _transposed(dev, c["kernel"], 9, cin, f)
    aff = (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g, short=None):
        cut = _cut(short)
        src, dz = g.inp(to_cn(c["du"])[:, :cut("ld_src", no)]), g.out("dz", cin, cut("ld_out", n))
        aux = g.inp(to_cn(c["x"])[:, :cut("ld_aux", n)])
        assert ops.split_applicable(L.SAR_CONV_TEMPORAL, 25, f, cin, 9, s, None, None, True, c["pad"])
        pm = ops.conv_gemm(L.SAR_CONV_TEMPORAL, src, dz, wT, f * cin, cin, B=B, V=25, T_src=To, T_out=T, Kc=f, M=cin, taps=9, stride=s,
                           pad=c["pad"], transposed=True, epi=L.SAR_EPI_MASK, aux=aux, aux_affine=aff, split=arith)
        g.part("mask", pm[0])
        g.ref("temporal data gradient", dz, to_cn(c["g_pre"]), TOL)
        g.ref("sum dz", lambda: pm[0].double().sum(dim=1)[:, 0], c["g_pre"].sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum dz x", lambda: pm[0].double().sum(dim=1)[:, 1], (c["g_pre"] * c["x"]).sum(dim=(0, 2, 3)), 1e-4)
    return fn


def temporal_weight_gradient(dev, arith, B, cin, f, T, s, more_splits=False):
    """conv_wgrad_ring_kernel (SAR_WGRAD_RING=0: conv_wgrad_split_kernel), wk = 2 (M <= 64) / 1, behind the folded prologue.
    more_splits: an explicit nsplit of more groups than there are tiles -- the empty ones must write zeros"""
    from sar_amd import ops, _lib as L
    c = temporal_case(B, cin, f, T, s)
    To, n, no, ws = c["To"], B * T * 25, B * c["To"] * 25, 9 * cin * f
    pro = (c["sc"].to(dev), c["sh"].to(dev))
    geo = dict(B=B, T_src=T, T_out=To, Kc=cin, M=f, taps=9, stride=s, pad=c["pad"])

    def fn(g, short=None):
        cut = _cut(short)
        src, dout = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.inp(to_cn(c["du"])[:, :cut("ld_dout", no)])
        flat = g.flat("dW | dbias", ws + f)
        blocks, wk, _ = _wgrad_blocks(arith, L.SAR_CONV_TEMPORAL, src, dout, pro=pro, **geo)
        assert blocks > 0 and wk == (2 if f <= 64 else 1)
        ops.conv_wgrad(L.SAR_CONV_TEMPORAL, src, dout, flat, V=25, pro=pro, pro_relu=True, w_stride_tap=cin * f, w_stride_c=f, wsize=ws,
                       bsize=f, split=arith, slabs=g.slab_batch(_slab_reduce), nsplit=wk * (B * To + 3) - 1 if more_splits else None, **geo)
        g.ref("temporal dW", lambda: flat[:ws].cpu().view(9, 1, cin, f), c["g_k"], TOL)
        g.ref("temporal dbias", lambda: flat[ws:], c["g_b"], TOL)
    return fn


# (B, cin, f, T, s): n % 4 == 0 at 2 x 14, n odd at 3 x 13; two tiles per sequence with a ragged second one (FT = 10 frames)
T_FORWARD = [(2, 64, 64, 14, 1), (3, 64, 64, 13, 2), (3, 20, 72, 13, 1), (2, 8, 64, 14, 2)]
# TR 1 at stride 1; TR 3 at stride 2 with T_out = 14 (even) and 13 (odd); Kc = f: 64, 20 (a ragged last group), 8; M = cin: 64, 72
T_DGRAD = [(2, 64, 64, 14, 1), (3, 72, 20, 13, 1), (2, 64, 64, 14, 2), (3, 72, 8, 13, 2), (3, 64, 20, 13, 2)]
# stride 2 is built for pad 3 and T_src = 2 T_out (even T); wk = 2 at M = f <= 64, wk = 1 at 72
T_WGRAD = [(2, 64, 64, 14, 1), (3, 64, 72, 13, 1), (3, 20, 64, 13, 1), (2, 64, 64, 14, 2), (2, 20, 72, 14, 2)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T,s", T_FORWARD)
def test_temporal_conv_forward_fused_prologue_and_stats(dev, B, cin, f, T, s, arith, pad):
    _drive(dev, temporal_forward(dev, arith, B, cin, f, T, s), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T,s", T_DGRAD)
def test_temporal_conv_data_gradient_masked(dev, B, cin, f, T, s, arith, pad):
    _drive(dev, temporal_data_gradient(dev, arith, B, cin, f, T, s), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T,s", T_WGRAD)
def test_temporal_weight_gradient(dev, B, cin, f, T, s, arith, pad):
    _drive(dev, temporal_weight_gradient(dev, arith, B, cin, f, T, s), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T,s", [(2, 64, 64, 14, 1), (2, 20, 72, 14, 2)])
def test_temporal_weight_gradient_with_empty_splits(dev, B, cin, f, T, s, arith, pad):
    _drive(dev, temporal_weight_gradient(dev, arith, B, cin, f, T, s, more_splits=True), pad)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_out", "ld_aux"])
@pytest.mark.parametrize("s", [1, 2])
def test_temporal_conv_rejects_a_leading_dimension_below_the_live_width(dev, s, short, arith):
    if short != "ld_aux":
        _rejected(dev, temporal_forward(dev, arith, 2, 64, 64, 14, s), short)
    _rejected(dev, temporal_data_gradient(dev, arith, 2, 64, 64, 14, s), short)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_dout"])
@pytest.mark.parametrize("s", [1, 2])
def test_temporal_weight_gradient_rejects_a_leading_dimension_below_the_live_width(dev, s, short, arith):
    _rejected(dev, temporal_weight_gradient(dev, arith, 2, 64, 64, 14, s), short)


# ------------------------------------------------------------------------------------------------ the 1-tap operator
@functools.lru_cache(maxsize=None)
def one_tap_case(B, cin, f, T, s):
    """the strided 1x1 residual convolution (tests/test_gpu_split.py: test_one_tap_temporal_operator_on_the_split_kernel)"""
    g = torch.Generator().manual_seed(cin * 7 + f + T + s)
    x = torch.randn(B, cin, T, 25, generator=g).double().requires_grad_(True)
    kernel = (torch.randn(1, 1, cin, f, generator=g) * 0.1).double().requires_grad_(True)
    bias = (torch.randn(f, generator=g) * 0.1).double().requires_grad_(True)
    y = F.conv2d(x, O.hwio_to_oihw(kernel), bias, stride=(s, 1))
    To = y.shape[2]
    dr = torch.randn(B, f, To, 25, generator=g)
    gk, gb = torch.autograd.grad(y, (kernel, bias), dr.double())
    no = B * To * 25
    add, aux = torch.randn(f, no, generator=g), torch.randn(f, no, generator=g)
    asc, ash = 1 + 0.1 * torch.randn(f, generator=g), 0.1 * torch.randn(f, generator=g)
    return dict(x=x.detach(), kernel=kernel.detach(), bias=bias.detach(), y=y.detach(), To=To, dr=dr, gk=gk, gb=gb, add=add, aux=aux,
                asc=asc, ash=ash)


def one_tap_forward(dev, arith, B, cin, f, T, s, epi):
    """conv_tap1_split_kernel with the STATS / ADD / MASK epilogue"""
    from sar_amd import ops, _lib as L
    c = one_tap_case(B, cin, f, T, s)
    To, n, no = c["To"], B * T * 25, B * c["To"] * 25
    W, bias = c["kernel"].float().to(dev), c["bias"].float().to(dev)
    yc = to_cn(c["y"])

    def fn(g, short=None):
        cut = _cut(short)
        src, out = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.out("out", f, cut("ld_out", no))
        kw = {}
        if epi == "add":
            kw = dict(epi=L.SAR_EPI_ADD, aux=g.inp(c["add"][:, :cut("ld_aux", no)]))
        elif epi == "mask":
            kw = dict(epi=L.SAR_EPI_MASK, aux=g.inp(c["aux"][:, :cut("ld_aux", no)]), aux_affine=(c["asc"].to(dev), c["ash"].to(dev)))
        else:
            kw = dict(epi=L.SAR_EPI_STATS)
        assert ops.split_applicable(L.SAR_CONV_TEMPORAL, 25, cin, f, 1, s, None, None, False, 0)
        r = ops.conv_gemm(L.SAR_CONV_TEMPORAL, src, out, W, 0, f, B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s, pad=0,
                          bias=bias, split=arith, **kw)
        if epi == "stats":
            g.part("stats", r[0])
            g.ref("1-tap forward", out, yc, TOL)
            g.ref("sum", lambda: r[0].double().sum(dim=1)[:, 0], yc.sum(dim=1), 1e-4)
            g.ref("sum of squares", lambda: r[0].double().sum(dim=1)[:, 1], (yc * yc).sum(dim=1), TOL)
        elif epi == "add":
            g.ref("1-tap forward + aux", out, yc + c["add"].double(), TOL)
        else:
            want = yc * ((c["aux"].double() * c["asc"].double().view(-1, 1) + c["ash"].double().view(-1, 1)) > 0)
            g.part("mask", r[0])
            g.ref("1-tap forward, masked", out, want, TOL)
            g.ref("sum out", lambda: r[0].double().sum(dim=1)[:, 0], want.sum(dim=1), 1e-4)
    return fn


def one_tap_weight_gradient(dev, arith, B, cin, f, T, s, more_splits=False):
    """wgrad_tap1_split_kernel (T_src = stride T_out)"""
    from sar_amd import ops, _lib as L
    c = one_tap_case(B, cin, f, T, s)
    To, n, no = c["To"], B * T * 25, B * c["To"] * 25
    geo = dict(B=B, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s, pad=0)

    def fn(g, short=None):
        cut = _cut(short)
        src, dout = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.inp(to_cn(c["dr"])[:, :cut("ld_dout", no)])
        flat = g.flat("dW | dbias", cin * f + f)
        blocks, wk, _ = _wgrad_blocks(arith, L.SAR_CONV_TEMPORAL, src, dout, **geo)
        assert blocks > 0 and wk == 1
        ops.conv_wgrad(L.SAR_CONV_TEMPORAL, src, dout, flat, V=25, w_stride_tap=0, w_stride_c=f, wsize=cin * f, bsize=f, split=arith,
                       slabs=g.slab_batch(_slab_reduce), nsplit=B * To + 3 if more_splits else None, **geo)
        g.ref("1-tap dW", lambda: flat[:cin * f].cpu().view(1, 1, cin, f), c["gk"], TOL)
        g.ref("1-tap dbias", lambda: flat[cin * f:], c["gb"], TOL)
    return fn


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("epi", ["stats", "add", "mask"])
@pytest.mark.parametrize("B,cin,f,T,s", [(2, 20, 64, 14, 1), (3, 40, 72, 13, 2), (3, 20, 64, 13, 2)])
def test_one_tap_forward(dev, B, cin, f, T, s, epi, arith, pad):
    _drive(dev, one_tap_forward(dev, arith, B, cin, f, T, s, epi), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T,s,more", [(3, 20, 64, 13, 1, False), (2, 40, 72, 14, 2, False), (2, 40, 72, 14, 2, True)])
def test_one_tap_weight_gradient(dev, B, cin, f, T, s, more, arith, pad):
    _drive(dev, one_tap_weight_gradient(dev, arith, B, cin, f, T, s, more), pad)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_out", "ld_aux", "ld_dout"])
def test_one_tap_rejects_a_leading_dimension_below_the_live_width(dev, short, arith):
    if short == "ld_dout":
        _rejected(dev, one_tap_weight_gradient(dev, arith, 2, 40, 72, 14, 2), short)
        return
    _rejected(dev, one_tap_forward(dev, arith, 2, 40, 72, 14, 2, "mask"), short)
    if short == "ld_src":
        _rejected(dev, one_tap_weight_gradient(dev, arith, 2, 40, 72, 14, 2), short)


# ------------------------------------------------------------------------------------------------ the graph operator
@functools.lru_cache(maxsize=None)
def graph_case(B, cin, f, T):
    """GraphConvTD and its gradients in float64 (tests/test_gpu_guard_bands.py: graph_case, at the channel counts of this family)"""
    g = torch.Generator().manual_seed(7 * cin + f + 1000 * B + T)
    x = torch.randn(B, cin, T, 25, generator=g).double().requires_grad_(True)
    kernel = (torch.randn(1, 1, cin, 3 * f, generator=g) * 0.1).double().requires_grad_(True)
    bias = (torch.randn(3 * f, generator=g) * 0.1).double().requires_grad_(True)
    dout = torch.randn(B, f, T, 25, generator=g)
    y = O.graph_conv_td(x, kernel, bias, _A().double())
    gx, gk, gb = torch.autograd.grad(y, (x, kernel, bias), dout.double())
    n = B * T * 25
    extra = dict(add=torch.randn(cin, n, generator=g), u=torch.randn(cin, n, generator=g), mean=0.1 * torch.randn(cin, generator=g),
                 keep=torch.rand(cin, n, generator=g) > 0.4, compact=torch.randn(cin, B * ((T + 1) // 2) * 25, generator=g),
                 aux=torch.randn(cin, n, generator=g), asc=1 + 0.1 * torch.randn(cin, generator=g), ash=0.2 * torch.randn(cin, generator=g),
                 gamma=1 + 0.1 * torch.randn(f, generator=g), beta=0.1 * torch.randn(f, generator=g))
    return dict(x=x.detach(), kernel=kernel.detach(), bias=bias.detach(), dout=dout, y=y.detach(), gx=gx, gk=gk, gb=gb, **extra)


def graph_forward(dev, arith, B, cin, f, T):
    """conv_graph_split_kernel (SAR_GRAPH_SPLIT2=1, f16x3a: conv_graph_split2_kernel<STATS>): forward with bias and the STATS epilogue"""
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n = B * T * 25
    W, bias = c["kernel"].float().to(dev), c["bias"].float().to(dev)

    def fn(g, short=None):
        cut = _cut(short)
        src, out = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.out("out", f, cut("ld_out", n))
        assert ops.split_applicable(L.SAR_CONV_GRAPH, 25, cin, f, 3, 1, _tables(), None, False, 0)
        r = ops.conv_gemm(L.SAR_CONV_GRAPH, src, out, W, f, 3 * f, B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f, taps=3, bias=bias,
                          tables=_tables(), epi=L.SAR_EPI_STATS, split=arith)
        g.part("stats", r[0])
        z = lambda: torch.empty(f, device=dev)
        mean, rstd, scale, shift = z(), z(), z(), z()
        ops.bn_finalize(r[0], r[1], f, n, 1e-3, 0.99, True, c["gamma"].to(dev), c["beta"].to(dev), torch.zeros(f, device=dev),
                        torch.ones(f, device=dev), mean, rstd, scale, shift)
        g.ref("graph forward", out, to_cn(c["y"]), TOL)
        g.ref("mean of the epilogue partials", mean, c["y"].mean(dim=(0, 2, 3)), TOL)
        g.ref("rstd of the epilogue partials", rstd, torch.rsqrt(c["y"].var(dim=(0, 2, 3), unbiased=False) + 1e-3), TOL)
    return fn


def graph_data_gradient(dev, arith, B, cin, f, T, epi):
    """the data gradient on the transposed tables (Kc = f, M = cin): conv_graph_split2_kernel<EPI> in f16x3a -- and once more with
    ops.GRAPH_ONE_TILE_WG on conv_graph_split_kernel, which must give EQUAL bits at every pad --, conv_graph_split_kernel in bf16x6.
    epi: none | mask | add | gate | even (ADD with SAR_GRAPH_AUX_EVEN_FRAMES: the compact aux of the even frames)"""
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n, Ta = B * T * 25, (T + 1) // 2
    gT = _transposed(dev, c["kernel"], 1, cin, 3 * f).view(3 * f, cin)
    gx = to_cn(c["gx"])
    full = torch.zeros(cin, B, T, 25)
    full[:, :, 0::2] = c["compact"].view(cin, B, Ta, 25)
    full = full.reshape(cin, n).double()
    keep_mask = (c["aux"].double() * c["asc"].double().view(-1, 1) + c["ash"].double().view(-1, 1)) > 0

    def fn(g, short=None):
        cut = _cut(short)
        src = g.inp(to_cn(c["dout"])[:, :cut("ld_src", n)])
        kw = {}
        if epi == "mask":
            kw = dict(epi=L.SAR_EPI_MASK, aux=g.inp(c["aux"][:, :cut("ld_aux", n)]), aux_affine=(c["asc"].to(dev), c["ash"].to(dev)),
                      aux_mean=c["mean"].to(dev))
        elif epi == "add":
            kw = dict(epi=L.SAR_EPI_ADD, aux=g.inp(c["add"][:, :cut("ld_aux", n)]))
        elif epi == "even":
            kw = dict(epi=L.SAR_EPI_ADD, aux=g.inp(c["compact"][:, :cut("ld_aux", B * Ta * 25)]), aux_even_frames=True)
        elif epi == "gate":
            n2 = cut("ld_aux2", n)
            kw = dict(epi=L.SAR_EPI_ADD_GATE, aux=g.inp(c["add"][:, :cut("ld_aux", n)]), aux2=g.inp(c["u"][:, :n2]),
                      aux_mask=g.mask("keep", cin, n2, c["keep"][:, :n2].contiguous()), aux_mean=c["mean"].to(dev))
        assert ops.split_applicable(L.SAR_CONV_GRAPH, 25, f, cin, 3, 1, _tables(True), None, False, 0)
        res = []
        for name in ("dx", "dx (one tile per workgroup)") if arith == "f16x3a" else ("dx",):
            out = g.out(name, cin, cut("ld_out", n))
            ops.GRAPH_ONE_TILE_WG = name != "dx"
            try:
                r = ops.conv_gemm(L.SAR_CONV_GRAPH, src, out, gT, f * cin, cin, B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3,
                                  tables=_tables(True), split=arith, **kw)
            finally:
                ops.GRAPH_ONE_TILE_WG = False
            if r is not None:
                g.part(name, r[0])
            res.append((out, r))
        dx, pm = res[0]
        if len(res) == 2:
            g.ref("one tile per workgroup == persistent", res[1][0], dx, 0)
            if pm is not None:
                g.ref("one tile per workgroup == persistent: partials", res[1][1][0], pm[0], 0)
        if epi == "none":
            g.ref("graph data gradient", dx, gx, TOL)
        elif epi == "mask":
            want = gx * keep_mask
            g.ref("graph data gradient, masked", dx, want, TOL)
            g.ref("sum dz", lambda: pm[0].double().sum(dim=1)[:, 0], want.sum(dim=1), 1e-4)
            g.ref("sum dz (aux - mean)", lambda: pm[0].double().sum(dim=1)[:, 1],
                  (want * (c["aux"].double() - c["mean"].double().view(-1, 1))).sum(dim=1), 1e-4)
        elif epi == "add":
            g.ref("graph data gradient + aux", dx, gx + c["add"].double(), TOL)
        elif epi == "even":
            g.ref("graph data gradient + even-frame skip", dx, gx + full, TOL)
        else:
            g.ref("gated data gradient", dx, torch.where(c["keep"], gx + c["add"].double(), torch.zeros(1, dtype=torch.float64)), TOL)
            g.ref("sum out", lambda: pm[0].double().sum(dim=1)[:, 0], lambda: dx.double().sum(dim=1), 1e-6)
            g.ref("sum out (aux2 - mean)", lambda: pm[0].double().sum(dim=1)[:, 1],
                  lambda: (dx.double().cpu() * (c["u"].double() - c["mean"].double().view(-1, 1))).sum(dim=1), 1e-6)
    return fn


def graph_weight_gradient(dev, arith, B, cin, f, T, identity=True, more_splits=False):
    """graph_wgrad_split_kernel, wk = 4 (M <= 64) / 2 (M <= 128) / 1; identity: with SAR_GRAPH_SLICE0_IDENTITY (the raw tile through
    LDS for slice 0) as the engines' tables carry it, or without"""
    from sar_amd import ops, _lib as L
    c = graph_case(B, cin, f, T)
    n, ws, bs = B * T * 25, cin * 3 * f, 3 * f
    tables = _tables()
    assert tables.g_flags & L.SAR_GRAPH_SLICE0_IDENTITY
    if not identity:
        tables = copy.copy(tables)
        tables.g_flags &= ~L.SAR_GRAPH_SLICE0_IDENTITY
    geo = dict(B=B, T_src=T, T_out=T, Kc=cin, M=f, taps=3)

    def fn(g, short=None):
        cut = _cut(short)
        src, dout = g.inp(to_cn(c["x"])[:, :cut("ld_src", n)]), g.inp(to_cn(c["dout"])[:, :cut("ld_dout", n)])
        flat = g.flat("dW | dbias", ws + bs)
        blocks, wk, _ = _wgrad_blocks(arith, L.SAR_CONV_GRAPH, src, dout, tables=tables, **geo)
        assert blocks > 0 and wk == (4 if f <= 64 else 2 if f <= 128 else 1)
        ops.conv_wgrad(L.SAR_CONV_GRAPH, src, dout, flat, V=25, tables=tables, w_stride_tap=f, w_stride_c=3 * f, wsize=ws, bsize=bs,
                       split=arith, slabs=g.slab_batch(_slab_reduce), nsplit=wk * (B * T + 3) - 1 if more_splits else None, **geo)
        g.ref("graph dW", lambda: flat[:ws].cpu().view(1, 1, cin, 3 * f), c["gk"], TOL)
        g.ref("graph dbias", lambda: flat[ws:], c["gb"], TOL)
    return fn


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T", [(2, 16, 64, 14), (3, 32, 72, 13)])
def test_graph_conv_forward_with_stats(dev, B, cin, f, T, arith, pad):
    _drive(dev, graph_forward(dev, arith, B, cin, f, T), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("epi", ["none", "mask", "add", "even"])
@pytest.mark.parametrize("B,cin,f,T", [(2, 64, 16, 14), (3, 72, 32, 13)])
def test_graph_data_gradient(dev, B, cin, f, T, epi, arith, pad):
    """Kc = 16 (the minimum) and 32, M = 64 and 72 (a ragged second row block), two tiles per sequence, row starts of every 4-byte
    phase at 3 x 13 frames with pad 7"""
    _drive(dev, graph_data_gradient(dev, arith, B, cin, f, T, epi), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("B,cin,f,T", [(2, 64, 16, 14), (2, 72, 32, 14)])
def test_graph_data_gradient_gated_epilogue(dev, B, cin, f, T, arith, pad):
    """SAR_EPI_ADD_GATE with aux, aux2 and the mask bytes guarded; ld_aux2 % 4 != 0 (pad = 7) is rejected"""
    fn = graph_data_gradient(dev, arith, B, cin, f, T, "gate")
    if pad % 4:
        rejected(dev, fn, pad, launch=SplitLaunch)
        return
    _drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("B,cin,f,T", [(2, 16, 64, 14), (3, 32, 72, 13), (2, 16, 136, 14)])
def test_graph_weight_gradient(dev, B, cin, f, T, identity, arith, pad):
    _drive(dev, graph_weight_gradient(dev, arith, B, cin, f, T, identity), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
def test_graph_weight_gradient_with_empty_splits(dev, arith, pad):
    _drive(dev, graph_weight_gradient(dev, arith, 2, 16, 64, 14, more_splits=True), pad)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_out"])
def test_graph_forward_rejects_a_leading_dimension_below_the_live_width(dev, short, arith):
    _rejected(dev, graph_forward(dev, arith, 2, 16, 64, 14), short)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("epi,short", [("none", "ld_src"), ("none", "ld_out"), ("mask", "ld_src"), ("mask", "ld_out"), ("mask", "ld_aux"),
                                       ("add", "ld_src"), ("add", "ld_out"), ("add", "ld_aux"), ("even", "ld_src"), ("even", "ld_out"),
                                       ("even", "ld_aux"), ("gate", "ld_src"), ("gate", "ld_out"), ("gate", "ld_aux"), ("gate", "ld_aux2")])
def test_graph_data_gradient_rejects_a_leading_dimension_below_the_live_width(dev, epi, short, arith):
    _rejected(dev, graph_data_gradient(dev, arith, 2, 64, 16, 14, epi), short)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_dout"])
@pytest.mark.parametrize("f", [64, 72, 136])
def test_graph_weight_gradient_rejects_a_leading_dimension_below_the_live_width(dev, f, short, arith):
    _rejected(dev, graph_weight_gradient(dev, arith, 2, 16, f, 14), short)


# ------------------------------------------------------------------------------------------------ sar_conv2d_gemm_split / _wgrad_split
@functools.lru_cache(maxsize=None)
def conv2d_case(cin, cout, H, W, B):
    """3x3 / stride 1 / pad 1 behind a folded BatchNorm + ReLU and its gradients (tests/test_gpu_split.py:
    test_conv2d_3x3_forward_and_masked_data_gradient / test_conv2d_3x3_weight_gradient) in float64"""
    g = torch.Generator().manual_seed(cin + 3 * cout + H + B)
    x = torch.randn(B, cin, H, W, generator=g).double()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).double().requires_grad_(True)
    sc, sh = (1 + 0.2 * torch.randn(cin, generator=g)).double(), (0.3 * torch.randn(cin, generator=g)).double()
    hin = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    y = F.conv2d(hin, w, None, stride=1, padding=1)
    dy = torch.randn(y.shape, generator=g).double()
    gh, gw = torch.autograd.grad(y, (hin, w), dy)
    aux = torch.randn(cin, B * H * W, generator=g)
    asc, ash, amu = 1 + 0.1 * torch.randn(cin, generator=g), 0.2 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    return dict(x=x, w=w.detach(), sc=sc.float(), sh=sh.float(), y=y.detach(), dy=dy, gh=gh, gw=gw, aux=aux, asc=asc, ash=ash, amu=amu)


def _kslab(g):
    """the K-split workspace as a guarded flat range (ops.conv2d_gemm: kslab=)"""
    def alloc(nfloats):
        assert not g.kslabs, "one workspace per launch"
        g.kslabs.append(guarded_flat(nfloats, SENTINEL, g.dev, 8))
        return g.kslabs[0][0]
    return alloc


def _variant0():
    return os.environ.get("SAR_C2S_VARIANT") == "0"      # (pick_variant: the three-per-CU kernel has no K-split)


def conv2d_forward(dev, arith, cin, cout, H, W, B, nparts=None):
    """conv2d_split_kernel: forward behind the folded prologue with the STATS epilogue.  nparts: (K-split, one pass) where the shape
    plans a K-split -- taken when ld_out % 4 == 0 (pick_variant), else the launch drops to one pass and must say so in nparts"""
    from sar_amd import ops, _lib as L
    c = conv2d_case(cin, cout, H, W, B)
    n = B * H * W
    geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=W, H_out=H, W_out=W, KH=3, KW=3, stride=1, pad=1)
    wf = c["w"].float().permute(2, 3, 1, 0).reshape(-1).contiguous().to(dev)          # (tap, c, m)
    pro = (c["sc"].to(dev), c["sh"].to(dev))
    yc = cn(c["y"])

    def fn(g, short=None):
        cut = _cut(short)
        g.kslabs = []
        src, out = g.inp(cn(c["x"])[:, :cut("ld_src", n)]), g.out("out", cout, cut("ld_out", n))
        assert ops.conv2d_split_applicable(**geo)
        r = ops.conv2d_gemm(src, out, wf, cin * cout, cout, epi=L.SAR_EPI_STATS, pro=pro, pro_relu=True, split=arith,
                            kslab=_kslab(g), **geo)
        if nparts is not None and short is None:
            one_pass = bool(g.pad % 4) or _variant0()
            assert r[1] == nparts[one_pass], "nparts %d at pad %d" % (r[1], g.pad)
            assert len(g.kslabs) == (0 if _variant0() else 1)
        g.part("stats", r[0])
        g.ref("conv2d forward", out, yc, TOL)
        g.ref("sum", lambda: r[0].double().sum(1)[:, 0], yc.sum(1), TOL, scale=yc.abs().sum(1).max().item())
        g.ref("sum of squares", lambda: r[0].double().sum(1)[:, 1], (yc * yc).sum(1), TOL)
        g.ref("K-split workspace guards", lambda: _kslab_guards(g), torch.ones(1, dtype=torch.bool), 0)
    return fn


def _kslab_guards(g):
    for _, whole in g.kslabs:
        assert_flat_guards_untouched(whole, whole.numel() - 16, SENTINEL, 8, "K-split workspace (pad %d)" % g.pad)
    return torch.ones(1, dtype=torch.bool)


def conv2d_data_gradient(dev, arith, cin, cout, H, W, B, nparts=None):
    """conv2d_split_kernel: the stride-1 data gradient (Kc = cout, M = cin, mirrored taps) with the MASK epilogue and its centred sums"""
    from sar_amd import ops, _lib as L
    c = conv2d_case(cin, cout, H, W, B)
    n = B * H * W
    geo = dict(B=B, Kc=cout, M=cin, H_src=H, W_src=W, H_out=H, W_out=W, KH=3, KW=3, stride=1, pad=1, transposed=True)
    wb = c["w"].float().permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)          # (tap, m, c)
    want = cn(c["gh"]) * ((c["aux"].double() * c["asc"].double().view(-1, 1) + c["ash"].double().view(-1, 1)) > 0)

    def fn(g, short=None):
        cut = _cut(short)
        g.kslabs = []
        src, dx = g.inp(cn(c["dy"])[:, :cut("ld_src", n)]), g.out("dx", cin, cut("ld_out", n))
        aux = g.inp(c["aux"][:, :cut("ld_aux", n)])
        assert ops.conv2d_split_applicable(epi=L.SAR_EPI_MASK, **geo)
        r = ops.conv2d_gemm(src, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=aux, aux_affine=(c["asc"].to(dev), c["ash"].to(dev)),
                            aux_mean=c["amu"].to(dev), split=arith, kslab=_kslab(g), **geo)
        if nparts is not None and short is None:
            one_pass = bool(g.pad % 4) or _variant0()
            assert r[1] == nparts[one_pass], "nparts %d at pad %d" % (r[1], g.pad)
            assert len(g.kslabs) == (0 if _variant0() else 1)
        g.part("mask", r[0])
        g.ref("conv2d data gradient, masked", dx, want, TOL)
        g.ref("sum dz (aux - mean)", lambda: r[0].double().sum(1)[:, 1], (want * (c["aux"].double() - c["amu"].double().view(-1, 1))).sum(1), 5 * TOL)
        g.ref("K-split workspace guards", lambda: _kslab_guards(g), torch.ones(1, dtype=torch.bool), 0)
    return fn


def conv2d_weight_gradient(dev, arith, cin, cout, H, W, B):
    """conv_wgrad_split_kernel<AR, wk, 0, W>: widths 8 / 16, wk = 2 (M <= 64) / 1, behind the folded prologue"""
    import ctypes as C
    from sar_amd import ops, _lib as L
    c = conv2d_case(cin, cout, H, W, B)
    n = B * H * W
    geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=W, H_out=H, W_out=W, KH=3, KW=3, stride=1, pad=1)
    pro = (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g, short=None):
        cut = _cut(short)
        src, dout = g.inp(cn(c["x"])[:, :cut("ld_src", n)]), g.inp(cn(c["dy"])[:, :cut("ld_dout", n)])
        dW = g.flat("dW", 9 * cin * cout)
        wk = C.c_int(0)
        d = ops._conv2d_desc(src, pro=pro, pro_relu=True, **geo)
        assert L.load().sar_conv2d_wgrad_split_blocks(C.byref(d), L.SAR_SPLIT[arith], C.byref(wk), None) > 0
        assert wk.value == (2 if cout <= 64 else 1)
        ops.conv2d_wgrad(src, dout, dW, pro=pro, pro_relu=True, split=arith, slabs=g.slab_batch(_slab_reduce), **geo)
        g.ref("conv2d weight gradient", lambda: dW.cpu().view(3, 3, cin, cout).permute(3, 2, 0, 1), c["gw"], TOL)
    return fn


# several images per tile (rectangular; a batch that does not fill the last tile), B H W odd, two tiles per image
C2D_SHAPES = [(16, 8, 10, 12, 5), (16, 8, 5, 7, 3), (8, 16, 20, 16, 2)]
# (cin, cout, H, W, B): widths 8 and 16; M = cout <= 64 and 72; Kc = cin = 24
C2D_WGRAD = [(8, 16, 6, 8, 3), (24, 72, 5, 16, 2), (24, 16, 9, 16, 1)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("cin,cout,H,W,B", C2D_SHAPES)
def test_conv2d_forward_and_masked_data_gradient(dev, cin, cout, H, W, B, arith, pad):
    _drive(dev, conv2d_forward(dev, arith, cin, cout, H, W, B), pad)
    _drive(dev, conv2d_data_gradient(dev, arith, cin, cout, H, W, B), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
def test_conv2d_k_split(dev, arith, pad):
    """(128 -> 16, 8 x 8, B 2) forward and the data gradient of (16 -> 128): G = 16 channel groups on one tile, so pick_variant plans
    ksplit = 2 -- a second reduction pass over a workspace, nparts counted in 1024-column chunks (1) instead of per tile (4) -- and
    takes it only when ld_out % 4 == 0 and ld_aux % 4 == 0.  THE EXCEPTION TO 2: at pad = 7 the launch drops to the one-pass kernel,
    another summation order, so that case is held to 1 (and 3, 4) only, and must return the one-pass nparts; at pad = 4 the K-split
    runs on a guarded output, aux and workspace and equals the tight launch bit for bit.  (SAR_C2S_VARIANT=0 has no K-split: one pass
    at every pad, bitwise throughout.)"""
    bitwise = pad % 4 == 0 or _variant0()
    _drive(dev, conv2d_forward(dev, arith, 128, 16, 8, 8, 2, nparts=(1, 4)), pad, bitwise)
    _drive(dev, conv2d_data_gradient(dev, arith, 16, 128, 8, 8, 2, nparts=(1, 4)), pad, bitwise)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("cin,cout,H", [(16, 32, 12), (8, 16, 16)])
def test_conv2d_stride2_data_gradient(dev, cin, cout, H, arith, pad):
    """conv2d_split_dgrad_s2_kernel (geometry_2f): the MASK epilogue with its sums, and the compact aux at the even pixels"""
    _drive(dev, conv2d_stride2_data_gradient(dev, arith, cin, cout, H), pad)


def conv2d_stride2_data_gradient(dev, arith, cin, cout, H):
    from sar_amd import ops, _lib as L
    B = 3
    w, dy, gx, aux, sc, sh, mu, small, Ho = parity_case(cin, cout, H)
    wb = w.float().permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)               # (tap, m, c)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Ho, H_out=H, W_out=H, KH=3, KW=3, stride=2, pad=1, transposed=True)
    ref = cn(gx) * ((aux.double() * sc.double()[:, None] + sh.double()[:, None]) > 0)
    full = torch.zeros(B, cin, H, H, dtype=torch.float64)
    full[:, :, ::2, ::2] = small.double().reshape(cin, B, Ho, Ho).permute(1, 0, 2, 3)
    n, ns = B * H * H, B * Ho * Ho

    def fn(g, short=None):
        cut = _cut(short)
        src = g.inp(cn(dy)[:, :cut("ld_src", ns)])
        dx = g.out("dx", cin, cut("ld_out", n))
        assert ops.conv2d_split_applicable(epi=L.SAR_EPI_MASK, **geo) and ops.conv2d_split_applicable(epi=L.SAR_EPI_ADD, aux_even_pixels=True, **geo)
        r = ops.conv2d_gemm(src, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=g.inp(aux[:, :cut("ld_aux", n)]),
                            aux_affine=(sc.to(dev), sh.to(dev)), aux_mean=mu.to(dev), split=arith, **geo)
        g.part("mask", r[0])
        g.ref("masked data gradient", dx, ref, TOL)
        g.ref("sum dz", lambda: r[0].double().sum(1)[:, 0], ref.sum(1), 1e-4)
        g.ref("sum dz (aux - mean)", lambda: r[0].double().sum(1)[:, 1], (ref * (aux.double() - mu.double()[:, None])).sum(1), 1e-4)
        if short is None:
            dx2 = g.out("dx + even pixels", cin, n)
            ops.conv2d_gemm(src, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(small), aux_even_pixels=True, split=arith, **geo)
            g.ref("data gradient + compact aux", dx2, cn(gx + full), TOL)
    return fn


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("cin,cout,H,W,B", C2D_WGRAD)
def test_conv2d_weight_gradient(dev, cin, cout, H, W, B, arith, pad):
    _drive(dev, conv2d_weight_gradient(dev, arith, cin, cout, H, W, B), pad)


# ---- rectangular images (tests/conv2d_rect_cases.py): the two smallest cases of group A, and the cases of group F that
# sar_conv2d_wgrad_split_blocks accepts (3x3 / stride 1 at widths 64, 32, 16, 8; the stride-2 ones and the H / W twins stay fp32)
RECT_S2 = [(8, 16, 8, 36), (16, 32, 12, 20)]
RECT_WGRAD = [(cin, cout, H, W) for cin, cout, s, H, W in RC.F_ALL if s == 1 and W in (8, 16, 32, 64)]


def conv2d_stride2_data_gradient_rect(dev, arith, cin, cout, H, W):
    """conv2d_stride2_data_gradient on an H x W image with Ho != Wo"""
    from sar_amd import ops, _lib as L
    B = RC.A_BATCH
    c = RC.conv_ref(cin, cout, 3, 2, H, W, B)
    Ho, Wo = c["Ho"], c["Wo"]
    wb = c["w"].permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)                  # (tap, m, c)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Wo, H_out=H, W_out=W, KH=3, KW=3, stride=2, pad=1, transposed=True)

    def fn(g):
        src, dx = g.inp(cn(c["dy"])), g.out("dx", cin, B * H * W)
        assert ops.conv2d_split_applicable(epi=L.SAR_EPI_MASK, **geo) and ops.conv2d_split_applicable(epi=L.SAR_EPI_ADD, aux_even_pixels=True, **geo)
        r = ops.conv2d_gemm(src, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=g.inp(c["aux"]),
                            aux_affine=(c["sc2"].to(dev), c["sh2"].to(dev)), aux_mean=c["mu"].to(dev), split=arith, **geo)
        g.part("mask", r[0])
        g.ref("masked data gradient", dx, c["dz"], TOL)
        g.ref("sum dz", lambda: r[0].double().sum(1)[:, 0], c["dz_sum"], 1e-4)
        g.ref("sum dz (aux - mean)", lambda: r[0].double().sum(1)[:, 1], c["dz_cen"], 1e-4)
        dx2 = g.out("dx + even pixels", cin, B * H * W)
        ops.conv2d_gemm(src, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=g.inp(c["small"]), aux_even_pixels=True, split=arith, **geo)
        g.ref("data gradient + compact aux", dx2, cn(c["gh_even"]), TOL)
    return fn


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("cin,cout,H,W", RECT_S2)
def test_conv2d_stride2_data_gradient_rectangular(dev, cin, cout, H, W, arith, pad):
    _drive(dev, conv2d_stride2_data_gradient_rect(dev, arith, cin, cout, H, W), pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("cin,cout,H,W", RECT_WGRAD)
def test_conv2d_weight_gradient_rectangular(dev, cin, cout, H, W, arith, pad):
    """widths 64, 32, 16 and 8 at heights 5, 6, 11 and 7"""
    assert len(RECT_WGRAD) == 4
    _drive(dev, conv2d_weight_gradient(dev, arith, cin, cout, H, W, 2), pad)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("short", ["ld_src", "ld_out", "ld_aux", "ld_dout"])
def test_conv2d_rejects_a_leading_dimension_below_the_live_width(dev, short, arith):
    if short == "ld_dout":
        _rejected(dev, conv2d_weight_gradient(dev, arith, 8, 16, 6, 8, 3), short)
        return
    if short != "ld_aux":
        _rejected(dev, conv2d_forward(dev, arith, 16, 8, 10, 12, 5), short)
        _rejected(dev, conv2d_forward(dev, arith, 128, 16, 8, 8, 2), short)
    _rejected(dev, conv2d_data_gradient(dev, arith, 16, 8, 10, 12, 5), short)
    _rejected(dev, conv2d_data_gradient(dev, arith, 16, 128, 8, 8, 2), short)
    _rejected(dev, conv2d_stride2_data_gradient(dev, arith, 16, 32, 12), short)
    if short == "ld_src":
        _rejected(dev, conv2d_weight_gradient(dev, arith, 8, 16, 6, 8, 3), short)


def test_conv2d_stride2_rejects_a_compact_aux_below_its_live_width(dev):
    """the SAR_C2D_AUX_EVEN_PIXELS launch alone: ld_aux = B Hc Wc - 1"""
    from sar_amd import ops, _lib as L
    cin, cout, H, B = 16, 32, 12, 3
    w, dy, gx, aux, sc, sh, mu, small, Ho = parity_case(cin, cout, H)
    wb = w.float().permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Ho, H_out=H, W_out=H, KH=3, KW=3, stride=2, pad=1, transposed=True)
    assert ops.conv2d_split_applicable(epi=L.SAR_EPI_ADD, aux_even_pixels=True, **geo)
    for arith in ARITHS:
        rejected(dev, lambda g: ops.conv2d_gemm(g.inp(cn(dy)), g.out("dx", cin, B * H * H), wb, cout * cin, cin, epi=L.SAR_EPI_ADD,
                                                aux=g.inp(small[:, :B * Ho * Ho - 1]), aux_even_pixels=True, split=arith, **geo),
                 0, launch=SplitLaunch)


# ------------------------------------------------------------------------------------------------ the bound producers
@pytest.mark.parametrize("pad", [0] + PADS)
@pytest.mark.parametrize("C,n", [(7, 1000), (5, 1001), (3, 9000)])
def test_amax_of_a_padded_view(dev, C, n, pad):
    """sar_amax_f32: the uint4 path (n % 4 == 0 and ld % 4 == 0: (7, 1000) and (3, 9000) at pad 0 / 4; 9000 columns are two chunks
    of 8192) and the scalar path (pad 7; n odd): the cell holds the bits of max |live| exactly -- the largest magnitude sits in the
    last column, the NaN of the padding right behind it --, is only ever raised, and ld = n - 1 is rejected"""
    from sar_amd import ops
    x = torch.randn(C, n, generator=torch.Generator().manual_seed(C + n))
    x[C // 2, n - 1] = -37.5
    xd = guarded(x, pad, NAN, dev, 4, 16)[0]
    cell = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.amax(xd, cell)
    assert _cell_bits(cell) == _bits(37.5)
    ops.amax(xd * 0.5, cell)
    assert _cell_bits(cell) == _bits(37.5)
    if pad == 0:
        cell.zero_()
        with pytest.raises(ops.L.SarError):
            ops.amax(torch.as_strided(xd, (C, n), (n - 1, 1)), cell)
        torch.cuda.synchronize()
        assert cell.item() == 0


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_bound_cells(dev, C, n, pad):
    """the amax_cell / amax_dr_cell by-products of bn_add_relu_fwd (with the mask where rows are 4-element groups, without
    one elsewhere: the pass itself raises the cell either way), bn_add_relu_bwd_apply and affine2: each cell holds the bits of max |live output| -- the same as the
    tight launch's, since the outputs are -- and the outputs do not depend on the cell being asked for"""
    from sar_amd import ops
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    yv = c["y"][2].float()
    kd = [d(v) for v in c["k"]]
    cells = {}

    def fn(g):
        cell = torch.zeros(4, dtype=torch.int32, device=dev)
        cells[g.pad] = cell
        u, r, dy = g.inp(c["u"]), g.inp(c["r"]), g.inp(c["dy"])
        masked = n % 4 == 0 and (n + g.pad) % 4 == 0
        y0, y1 = g.out("y", C, n), g.out("y (cell)", C, n)
        ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), 2, r, d(c["rsc"]), d(c["rsh"]), y0, mask=g.mask("relu 0", C, n) if masked else None)
        ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), 2, r, d(c["rsc"]), d(c["rsh"]), y1, mask=g.mask("relu 1", C, n) if masked else None,
                            amax_cell=cell[0:1])
        g.ref("y does not depend on the cell", y1, y0, 0)
        g.ref("y", y1, c["y"][2], TOL)
        if masked:
            g.ref("mask does not depend on the cell", lambda: g.masks["relu 1"][0], lambda: g.masks["relu 0"][0], 0)
        du0, dr0, dz0 = g.out("du", C, n), g.out("dr", C, n), g.out("dz", C, n)
        du1, dr1, dz1 = g.out("du (cell)", C, n), g.out("dr (cell)", C, n), g.out("dz (cell)", C, n)
        yin = g.inp(yv)
        m = g.mask("relu in", C, n, yv > 0) if masked else None
        ops.bn_add_relu_bwd_apply(dy, None if masked else yin, u, r, kd[:3], kd[3:], du0, dr0, dz0, mask=m)
        ops.bn_add_relu_bwd_apply(dy, None if masked else yin, u, r, kd[:3], kd[3:], du1, dr1, dz1, mask=m, amax_cell=cell[1:2],
                                  amax_dr_cell=cell[2:3])
        for a, b, name in ((du1, du0, "du"), (dr1, dr0, "dr"), (dz1, dz0, "dz")):
            g.ref("%s does not depend on the cells" % name, a, b, 0)
        a0, a1 = g.out("affine2", C, n), g.out("affine2 (cell)", C, n)
        ops.affine2(u, r, kd[:3], a0)
        ops.affine2(u, r, kd[:3], a1, amax_cell=cell[3:4])
        g.ref("affine2 does not depend on the cell", a1, a0, 0)
        for i, t in enumerate((y1, du1, dr1, a1)):
            g.ref("cell %d == bits of max |live output|" % i, lambda i=i: (cell[i:i + 1].cpu().to(torch.int64) & 0xffffffff),
                  lambda t=t: torch.tensor([_bits(t.abs().max().item())], dtype=torch.int64), 0)
    _drive(dev, fn, pad)
    assert torch.equal(cells[0], cells[pad]), "the cells of pad %d differ from the tight launch's" % pad


@pytest.mark.parametrize("which", ["fwd", "bwd_apply", "affine2"])
def test_block_tail_bound_cells_reject_a_leading_dimension_below_the_live_width(dev, which):
    """rows of n - 1 elements under a live width of n (the operands share one ld): nothing is written, the cells stay zero"""
    from sar_amd import ops
    C, n = 20, 776
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    kd = [d(v) for v in c["k"]]
    cell = torch.zeros(2, dtype=torch.int32, device=dev)
    short = lambda g, t: torch.as_strided(g.inp(t[:, :n - 1]), (C, n), (n - 1, 1))

    def fn(g):
        o = lambda name: torch.as_strided(g.out(name, C, n - 1), (C, n), (n - 1, 1))
        u, r = short(g, c["u"]), short(g, c["r"])
        mask = torch.zeros((C, n // 4), dtype=torch.uint8, device=dev)
        if which == "fwd":
            ops.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), 1, r, None, None, o("y"), mask=mask, amax_cell=cell[0:1])
        elif which == "bwd_apply":
            ops.bn_add_relu_bwd_apply(short(g, c["dy"]), None, u, r, kd[:3], kd[3:], o("du"), o("dr"), o("dz"), mask=mask,
                                      amax_cell=cell[0:1], amax_dr_cell=cell[1:2])
        else:
            ops.affine2(u, r, kd[:3], o("affine2"), amax_cell=cell[0:1])
    rejected(dev, fn, 0, launch=SplitLaunch)
    assert int(cell.abs().sum().item()) == 0


@pytest.mark.parametrize("arith", ARITHS)
def test_packed_split_weights_of_a_guarded_parameter_buffer(dev, arith):
    """sar_pack_weights_split_batch with a negative tap stride (the "mirror" item of ops._pack_split_conv2d) and with exchanged
    channel strides (a data gradient's view of the same tensor, Kc = 20: a ragged last group), from a flat parameter buffer whose
    tensors lie between NaN ranges, into an image between guards: every item's amax cell is exact (f16x3a: the x6 arithmetic has
    none), the image is bitwise that of a tight buffer, and the image's guards are untouched"""
    from sar_amd import ops
    g0 = torch.Generator().manual_seed(5)
    Kc, M = 24, 20
    w1, w2 = torch.randn(9 * Kc * M, generator=g0), torch.randn(9 * M * Kc, generator=g0) * 0.01
    w1[9 * Kc * M - 1], w2[0] = 5.5, -0.75
    gap = 8
    images, amaxes = [], []
    for guards in (False, True):
        if guards:
            flat, whole = guarded_flat(torch.cat([w1, torch.full((gap,), NAN), w2]), NAN, dev, 8)
            off2 = w1.numel() + gap
        else:
            flat, off2 = torch.cat([w1, w2]).to(dev), w1.numel()
        pk = ops.PackedSplitWeights(arith)
        pk.add("mirror", 8 * Kc * M, -Kc * M, M, 1, 9, Kc, M)              # element (tap, c, m) = w1[8 - tap][c][m]
        pk.add("exchanged", off2, M * Kc, 1, M, 9, M, Kc)                  # element (tap, c', m') = w2[tap][m'][c']: Kc' = 20, M' = 24
        pk.finalize(dev)
        if guards:
            nbytes = pk.buf.numel()
            pk.buf, image_whole = guarded_flat(nbytes, MASK_FILL, dev, 32, dtype=torch.uint8)
            assert pk.buf.data_ptr() % 16 == 0
        pk.refresh(flat)
        torch.cuda.synchronize()
        images.append(pk.buf.clone())
        amaxes.append(pk.amax.clone())
        if arith == "f16x3a":
            assert _cell_bits(pk.bound("mirror")) == _bits(5.5) and _cell_bits(pk.bound("exchanged")) == _bits(0.75)
    assert_flat_guards_untouched(image_whole, nbytes, MASK_FILL, 32, "weight image")
    assert torch.equal(images[0], images[1]), "the image of the guarded buffer differs from the tight buffer's"
    assert torch.equal(amaxes[0], amaxes[1])


@pytest.mark.parametrize("pad", [0] + PADS)
def test_slab_reduce_batch_with_strided_slabs_and_guarded_destinations(dev, pad):
    """sar_slab_reduce_batch_f32: two items of different length whose slabs are rows of stride n + pad between NaN, destinations
    between sentinels; bit-identical with sar_slab_reduce_f32 (ops.SlabBatch says so) and within the fp32 summation bound of the
    float64 sum: (nsplit - 1) roundings of 2^-24 on partial sums bounded by sum |x|"""
    from sar_amd import ops
    g0 = torch.Generator().manual_seed(pad)
    batch = ops.SlabBatch()
    g = SplitLaunch(dev, pad)
    items = []
    for name, nsplit, n in (("a", 5, 1003), ("b", 3, 40)):
        x = torch.randn(nsplit, n, generator=g0)
        slab = guarded(x, pad, NAN, dev, 4, 2)[0]
        out, single = g.flat(name, n), g.flat(name + " (single launch)", n)
        batch.add(slab, nsplit, n, out)
        _slab_reduce(slab, nsplit, n, single)
        items.append((x, out, single, nsplit))
    batch.flush()
    torch.cuda.synchronize()
    g.check()
    for x, out, single, nsplit in items:
        assert torch.equal(out, single)
        bound = (nsplit - 1) * 2.0 ** -24 * x.double().abs().sum(0)
        assert bool(((out.cpu().double() - x.double().sum(0)).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ the non-default paths
CONV_CASES = "temporal or one_tap or graph or conv2d"
CHILD_TIMEOUT = 60      # measured: 5.6 s per child (interpreter start-up, the float64 references, 300 cases), 4 s for the same cases in-process


def _child_pytest(env):
    """the convolution cases of this file in a fresh interpreter (the switches are read once per process), as
    tests/test_gpu_cn8_guard_bands.py: _child_pytest"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "(%s) and not non_default" % CONV_CASES], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT, cwd=ROOT)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (tail, r.stderr[-1500:])


def test_non_default_paths_persistent_forward_flat_window_and_three_per_cu(dev):
    """SAR_GRAPH_SPLIT2=1: conv_graph_split2_kernel<STATS> for the graph forward too (f16x3a); SAR_WGRAD_RING=0: conv_wgrad_split_kernel
    (the flat window) for the 9-tap weight gradients; SAR_C2S_VARIANT=0: conv2d_split_kernel<AR, 2, 0>, three workgroups per CU, no
    K-split"""
    _child_pytest(dict(SAR_GRAPH_SPLIT2="1", SAR_WGRAD_RING="0", SAR_C2S_VARIANT="0"))


def test_non_default_paths_double_buffered_256_pixel_tiles(dev):
    """SAR_C2S_VARIANT=1: conv2d_split_kernel<AR, 2, 1> (the small shapes of this file take variant 2 by default)"""
    _child_pytest(dict(SAR_C2S_VARIANT="1"))
