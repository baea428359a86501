"""Guard bands for the bf16 (CN8) kernels behind the C ABI ("The leading-dimension contract", CN8 table): every CN8
operand is a view into a larger bf16 allocation -- ld = n + pad units per plane, 2 planes in front and 2 behind -- whose every other
unit holds a known fill: NaN around inputs, -7.25 around outputs, 0xA5 around mask bytes.  Pad lanes (channels >= C of the last
plane) of an input are zero, the ABI's contract; those of an output start as the sentinel.  Each kernel runs tight (pad = 0, still
between guard planes), with pad = 1 (an off-by-one column lands in a guard) and with pad = 67 (odd, and longer than one 64-column
LDS-DMA piece); every unit is 16 bytes, so there is no aligned / unaligned split.  After each launch

  1. the live region meets the bar of the kernel's own test in tests/test_gpu_cn8.py on the same exact definitions (bf16 operands,
     float64 contraction): assert_bf16_close for stored tensors, 1e-4 for BatchNorm partial sums, 1e-5 for weight / bias gradients
     and pool_fwd, the gated epilogue's bars, torch.equal where that file asserts bit equality;
  2. the live region (outputs, masks, flat gradients, partials) is bitwise the tight launch's: no tile geometry depends on ld;
  3. every guard unit of every output and mask still holds its fill, bit for bit;
  4. every output, every partial and every returned reduction is finite: no NaN of an input's padding reached a result;
  5. pad lanes of every CN8 output are zero wherever C % 8 != 0;
  6. a leading dimension below the live width raises SarError and writes nothing.

The guards are part of the operand's own allocation, so a stray access shows as a failed assertion, never as a fault.  The
non-default staging paths (read once per process from the environment) run in two child pytest processes over this same file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stgcn as O
from util import (MASK_FILL, NAN, SENTINEL, assert_bf16_close, assert_cn8_guards_untouched, assert_cn8_pad_lanes_zero,
                  assert_flat_guards_untouched, assert_guards_untouched, bf, cn8_mask_bytes, cn8_values, graph_ref, guarded,
                  guarded_cn8, guarded_cn8_mask, guarded_flat, rel_err, to_cn)

pytestmark = pytest.mark.gpu
PADS = [1, 67]
FRONT, BACK, KFLAT = 2, 2, 8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = "bf16"                   # Launch.ref: a stored bf16 tensor (assert_bf16_close)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Launch:
    """the operands and results of one run of a case at one `pad`"""

    def __init__(self, dev, pad):
        self.dev, self.pad = dev, pad
        self.outs, self.flats, self.masks, self.parts, self.refs, self.rows = {}, {}, {}, {}, [], {}

    def inp(self, src, pad=None):
        """a (C, n) input of bf16-representable values as a guarded CN8 view: NaN all around, zero pad lanes"""
        return guarded_cn8(src.float(), self.pad if pad is None else pad, NAN, self.dev, FRONT, BACK)[0]

    def out(self, name, C, n, pad=None):
        view, whole = guarded_cn8((C, n), self.pad if pad is None else pad, SENTINEL, self.dev, FRONT, BACK)
        self.outs[name] = (view, whole, C, n)
        return view

    def values(self, name):
        """the (C, n) float32 values an output holds, on the host"""
        view, _, C, n = self.outs[name]
        return cn8_values(view[:, :n], C)

    def flat(self, name, n):
        view, whole = guarded_flat(n, SENTINEL, self.dev, KFLAT)
        self.flats[name] = (view, whole)
        return view

    def rows_out(self, name, C, n):
        """an fp32 (C, n) output with the fp32 guards of tests/test_gpu_guard_bands.py (the fp32 side of the layout conversion)"""
        view, whole = guarded((C, n), self.pad, SENTINEL, self.dev, 4, 2)
        self.rows[name] = (view, whole)
        return view

    def mask_in(self, mbytes, pad=None):
        """(G, n) gate bytes as a guarded (G, ld) input"""
        return guarded_cn8_mask(mbytes, self.pad if pad is None else pad, self.dev, FRONT, BACK)[0]

    def mask_out(self, name, C, n):
        G = (C + 7) // 8
        view, whole = guarded_cn8_mask((G, n), self.pad, self.dev, FRONT, BACK)
        self.masks[name] = (view, whole, G, n)
        return view

    def part(self, name, t, cols=None):
        """a reduction partial / returned reduction allocated outside the guards: checked finite and against the tight launch
        (cols: the leading entries of the last axis that are defined)"""
        self.parts[name] = t if cols is None else t[..., :cols]
        return t

    def ref(self, what, got, want, tol):
        """got (a tensor or a callable evaluated after the launches) against `want`: BF16 = assert_bf16_close, 0 = bitwise,
        else rel_err < tol"""
        self.refs.append((what, got, want, tol))

    def live(self):
        """name -> live region, of everything that is compared with the tight launch"""
        d = {}
        for name, (view, _, C, n) in self.outs.items():
            d["out " + name] = view[:, :n]
        for name, (view, _, G, n) in self.masks.items():
            d["mask " + name] = view[:, :n]
        for name, (view, _) in list(self.flats.items()) + list(self.rows.items()):
            d["flat " + name] = view
        for name, t in self.parts.items():
            d["partials " + name] = t
        return d

    def check(self):
        self.check_guards()                                                                      # 3
        for name, t in self.live().items():                                                      # 4
            if t.dtype != torch.uint8:
                assert bool(torch.isfinite(t.float()).all()), "%s (pad %d): not finite" % (name, self.pad)
        for name, (view, _, C, n) in self.outs.items():                                          # 5
            assert_cn8_pad_lanes_zero(view, C, n, "%s (pad %d)" % (name, self.pad))
        for what, got, want, tol in self.refs:                                                   # 1
            got = got() if callable(got) else got
            want = want() if callable(want) else want
            if tol == BF16:
                assert_bf16_close(got.cpu(), want.cpu(), "%s (pad %d)" % (what, self.pad))
            elif tol == 0:
                assert torch.equal(got.cpu(), want.cpu()), "%s (pad %d): not bitwise equal" % (what, self.pad)
            else:
                e = rel_err(got.cpu(), want.cpu())
                print("%s (pad %d): %.2e" % (what, self.pad, e))
                assert e < tol, "%s (pad %d): %.3e >= %.1e" % (what, self.pad, e, tol)

    def check_guards(self):
        for name, (view, whole, C, n) in self.outs.items():
            assert_cn8_guards_untouched(whole, C, n, SENTINEL, FRONT, BACK, "%s (pad %d)" % (name, self.pad))
        for name, (view, whole, G, n) in self.masks.items():
            assert_guards_untouched(whole, (G, n), MASK_FILL, FRONT, BACK, "mask %s (pad %d)" % (name, self.pad))
        for name, (view, whole) in self.flats.items():
            assert_flat_guards_untouched(whole, view.numel(), SENTINEL, KFLAT, "%s (pad %d)" % (name, self.pad))
        for name, (view, whole) in self.rows.items():
            assert_guards_untouched(whole, view.shape, SENTINEL, 4, 2, "%s (pad %d)" % (name, self.pad))

    def check_nothing_written(self):
        """6: a rejected call launched nothing"""
        for name, rec in list(self.outs.items()) + list(self.flats.items()) + list(self.rows.items()):
            assert bool((rec[1] == SENTINEL).all()), "%s (pad %d): written by a rejected call" % (name, self.pad)
        for name, rec in self.masks.items():
            assert bool((rec[1] == MASK_FILL).all()), "mask %s (pad %d): written by a rejected call" % (name, self.pad)


def drive(dev, fn, pad):
    """run `fn` tight and with `pad`, apply the five assertions"""
    tight, padded = Launch(dev, 0), Launch(dev, pad)
    fn(tight)
    fn(padded)
    torch.cuda.synchronize()
    tight.check()
    padded.check()
    a, b = tight.live(), padded.live()                                                           # 2
    assert set(a) == set(b)
    for name in b:
        assert torch.equal(a[name], b[name]), "%s: pad %d differs from the tight launch" % (name, pad)
    return tight, padded


def rejected(dev, fn):
    """the ABI does not take this leading dimension: the call raises SarError and writes nothing"""
    from sar_amd import _lib as L
    launch = Launch(dev, 0)
    with pytest.raises(L.SarError):
        fn(launch)
    torch.cuda.synchronize()
    launch.check_nothing_written()


def _A():
    from oracle.graph import spatial_adjacency
    return torch.tensor(spatial_adjacency().astype(np.float32))


@functools.lru_cache(maxsize=None)
def _tables(transpose=False, flags=True):
    """the NTU gather tables; flags=False: the same lists with g_flags = 0 (no SAR_GRAPH_FEW_DENSE: conv_graph_cn8_kernel builds every
    gathered tile)"""
    from sar_amd import ops
    from oracle.graph import spatial_adjacency
    t = ops.GraphTables(spatial_adjacency().astype(np.float32), torch.device("cuda:0"), transpose)
    if not flags:
        t.g_flags = 0
    return t


@functools.lru_cache(maxsize=None)
def _tables_general_slice0():
    from sar_amd import ops
    from oracle.graph import spatial_adjacency
    t = ops.GraphTables(spatial_adjacency().astype(np.float32), torch.device("cuda:0"), False)
    t.slice0_identity = False      # (g_flags stays as built, SAR_GRAPH_SLICE0_IDENTITY included: ops8.conv_wgrad passes this attribute on its own)
    return t


def _pack(W, st, sc, sm, taps, Kc, M):
    """the packed bf16 weight image (tests/test_gpu_cn8.py: _pack)"""
    from sar_amd import ops
    dev = torch.device("cuda:0")
    pk = ops.PackedWeights()
    pk.add("w", 0, st, sc, sm, taps, Kc, M)
    pk.finalize(dev)
    pk.refresh(W.float().to(dev).contiguous().reshape(-1))
    return pk.image("w")


def bf16r(*shape, g, scale=1.0):
    """seeded random values that a bf16 tensor holds exactly (float32)"""
    return (torch.randn(*shape, generator=g) * scale).bfloat16().float()


# ------------------------------------------------------------------------------------------------ sar_conv_gemm_cn8: temporal, 9 taps
# (B, f, T, s).  launch_by_m8<0, 9>: (2, 24, 9, 1) M <= 32 -> launch_cfg8<0, 9, 1, 2, 1, 4>, 3 planes; 64 channels -> <0, 9, 2, 2, 1, 4>
# (stride 1 and 2); (2, 72, 11, 1): M > 64 stays on <2, 2, 1, 4> (SAR_CN8_TILE default 2) with 9 planes -- the second plane of the
# last k-step (KC16) does not exist and Go is odd
TEMPORAL_FWD = [(2, 24, 9, 1), (2, 64, 13, 1), (3, 64, 14, 2), (2, 72, 11, 1)]


@functools.lru_cache(maxsize=None)
def temporal_fwd_case(B, f, T, s):
    """tests/test_gpu_cn8.py: test_temporal_conv_forward"""
    g = torch.Generator().manual_seed(f + T + s)
    x = bf16r(B, f, T, 25, g=g)
    sc = 1 + 0.2 * torch.randn(f, generator=g); sh = 0.3 * torch.randn(f, generator=g)
    kernel = torch.randn(9, 1, f, f, generator=g) * 0.05
    bias = torch.randn(f, generator=g) * 0.1
    h = torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))      # fp32 fma like the kernel
    ref = O.temporal_conv(bf(h), bf(kernel), bias.double(), s)
    To, pad, _ = O.same_pad(T, 9, s)
    return dict(x=x, sc=sc, sh=sh, bias=bias, ref=ref, To=To, pad=pad, pw=_pack(kernel, f * f, f, 1, 9, f, f))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", TEMPORAL_FWD)
def test_temporal_conv_forward_fused_prologue_and_stats(dev, B, f, T, s, pad):
    from sar_amd import ops8, _lib as L
    c = temporal_fwd_case(B, f, T, s)
    To, ref = c["To"], c["ref"]
    bias, pro = c["bias"].to(dev), (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g):
        out = g.out("out", f, B * To * 25)
        r = ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), out, c["pw"], B=B, V=25, T_src=T, T_out=To, Kc=f, M=f, taps=9,
                           stride=s, pad=c["pad"], bias=bias, pro=pro, pro_relu=True, epi=L.SAR_EPI_STATS)
        g.part("stats", r[0])
        g.ref("temporal forward", lambda: g.values("out"), to_cn(ref), BF16)
        g.ref("sum", lambda: r[0].double().sum(dim=1)[:, 0], ref.sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum of squares", lambda: r[0].double().sum(dim=1)[:, 1], (ref * ref).sum(dim=(0, 2, 3)), 1e-4)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def temporal_fwd_plain_case(B, f, T, s):
    g = torch.Generator().manual_seed(5 * f + T + s)
    x = bf16r(B, f, T, 25, g=g)
    kernel = torch.randn(9, 1, f, f, generator=g) * 0.05
    bias = torch.randn(f, generator=g) * 0.1
    To, pad, _ = O.same_pad(T, 9, s)
    return dict(x=x, bias=bias, ref=O.temporal_conv(x.double(), bf(kernel), bias.double(), s), To=To, pad=pad,
                pw=_pack(kernel, f * f, f, 1, 9, f, f))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", [(2, 24, 9, 1), (2, 64, 13, 1)])
def test_temporal_conv_forward_without_prologue(dev, B, f, T, s, pad):
    """The folded prologue of the cases above re-zeroes every staged unit outside the sequence (its keep mask), so a source descriptor
    that is one unit too long stays invisible there.  Without a prologue the staged units reach the matrix cores as loaded: the
    temporal zero padding behind the last frame of the last sequence is then the descriptor's range check alone."""
    from sar_amd import ops8, _lib as L
    c = temporal_fwd_plain_case(B, f, T, s)
    To, ref = c["To"], c["ref"]

    def fn(g):
        out = g.out("out", f, B * To * 25)
        ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), out, c["pw"], B=B, V=25, T_src=T, T_out=To, Kc=f, M=f, taps=9, stride=s,
                       pad=c["pad"], bias=c["bias"].to(dev))
        g.ref("temporal forward, no prologue", lambda: g.values("out"), to_cn(ref), BF16)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ 1 tap, forward and transposed
# (B, cin, f, T, s): launch_by_m8<0, 1> forward; transposed launch_by_m8<2, 1> (stride 2: generic-stride tap table) and <1, 1> (stride 1)
RESIDUAL = [(2, 24, 40, 9, 2), (1, 64, 64, 7, 1)]


@functools.lru_cache(maxsize=None)
def residual_case(B, cin, f, T, s):
    """tests/test_gpu_cn8.py: test_residual_conv_forward_and_data_gradient / test_residual_conv_weight_gradient"""
    g = torch.Generator().manual_seed(cin + f)
    x = bf16r(B, cin, T, 25, g=g)
    kernel = torch.randn(1, 1, cin, f, generator=g) * 0.1
    bias = torch.randn(f, generator=g) * 0.1
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, O.hwio_to_oihw(bf(kernel)), bias.double(), stride=(s, 1))
    To = ref.shape[2]
    dr = bf16r(B, f, To, 25, g=g)
    gx, = torch.autograd.grad(ref, xd, dr.double())
    k0 = torch.zeros(1, 1, cin, f, dtype=torch.float64, requires_grad=True)
    b0 = torch.zeros(f, dtype=torch.float64, requires_grad=True)
    gk, gb = torch.autograd.grad(F.conv2d(x.double(), O.hwio_to_oihw(k0), b0, stride=(s, 1)), (k0, b0), dr.double())
    return dict(x=x, bias=bias, ref=ref.detach(), To=To, dr=dr, gx=gx, gk=gk, gb=gb, pw=_pack(kernel, 0, f, 1, 1, cin, f),
                pwT=_pack(kernel, 0, 1, f, 1, f, cin))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T,s", RESIDUAL)
def test_residual_conv_forward_and_data_gradient(dev, B, cin, f, T, s, pad):
    from sar_amd import ops8, _lib as L
    c = residual_case(B, cin, f, T, s)
    To, ref = c["To"], c["ref"]

    def fn(g):
        out, dx = g.out("out", f, B * To * 25), g.out("dx", cin, B * T * 25)
        r = ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), out, c["pw"], B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=1,
                           stride=s, pad=0, bias=c["bias"].to(dev), epi=L.SAR_EPI_STATS)
        ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["dr"])), dx, c["pwT"], B=B, V=25, T_src=To, T_out=T, Kc=f, M=cin, taps=1,
                       stride=s, pad=0, transposed=True)
        g.part("stats", r[0])
        g.ref("residual forward", lambda: g.values("out"), to_cn(ref), BF16)
        g.ref("sum of squares", lambda: r[0].double().sum(dim=1)[:, 1], (ref ** 2).sum(dim=(0, 2, 3)), 1e-4)
        g.ref("residual data gradient", lambda: g.values("dx"), to_cn(c["gx"]), BF16)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ temporal data gradient, SAR_EPI_MASK
# (B, f, T, s).  launch_by_m8<1, 9> / <3, 9> / <2, 9>: (2, 64, 13, 1) -> conv_gemm_cn8_dma_kernel TR = 1; (2, 64, 14, 2), (2, 64, 11, 2)
# -> DMA TR = 3 (parity split), even and odd T; (2, 24, 9, 1), (2, 24, 10, 2): M <= 32 -> the register kernel launch_cfg8<1 / 3, 9, 1, 2,
# 1, 4>; (2, 64, 12, 3): TR = 2 (generic stride, never DMA); (2, 72, 11, 1): DMA TR = 1 with an odd plane count.  With SAR_CN8_DMA=0
# (the children below) the 64- and 72-channel cases run the register-staged / deep-prefetch kernels.
TEMPORAL_DGRAD = [(2, 64, 13, 1), (2, 64, 14, 2), (2, 64, 11, 2), (2, 24, 9, 1), (2, 24, 10, 2), (2, 64, 12, 3), (2, 72, 11, 1)]


@functools.lru_cache(maxsize=None)
def temporal_dgrad_case(B, f, T, s):
    """tests/test_gpu_cn8.py: test_temporal_conv_data_gradient"""
    g = torch.Generator().manual_seed(11 * f + T + s)
    gx = bf16r(B, f, T, 25, g=g)
    sc = 1 + 0.2 * torch.randn(f, generator=g); sh = 0.3 * torch.randn(f, generator=g); mean = 0.1 * torch.randn(f, generator=g)
    kernel = torch.randn(9, 1, f, f, generator=g) * 0.05
    To, pad, _ = O.same_pad(T, 9, s)
    du = bf16r(B, f, To, 25, g=g)
    h = torch.zeros(B, f, T, 25, dtype=torch.float64, requires_grad=True)
    dh, = torch.autograd.grad(O.temporal_conv(h, bf(kernel), None, s), h, du.double())
    pre = torch.addcmul(sh.view(1, -1, 1, 1), gx, sc.view(1, -1, 1, 1))
    g_pre = dh * (pre > 0)
    return dict(gx=gx, sc=sc, sh=sh, mean=mean, To=To, pad=pad, du=du, g_pre=g_pre, pw=_pack(kernel, f * f, 1, f, 9, f, f))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", TEMPORAL_DGRAD)
def test_temporal_conv_data_gradient_masked(dev, B, f, T, s, pad):
    from sar_amd import ops8, _lib as L
    c = temporal_dgrad_case(B, f, T, s)
    To, g_pre = c["To"], c["g_pre"]
    aff, mean = (c["sc"].to(dev), c["sh"].to(dev)), c["mean"].to(dev)

    def fn(g):
        dz = g.out("dz", f, B * T * 25)
        pm = ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["du"])), dz, c["pw"], B=B, V=25, T_src=To, T_out=T, Kc=f, M=f, taps=9,
                            stride=s, pad=c["pad"], transposed=True, epi=L.SAR_EPI_MASK, aux=g.inp(to_cn(c["gx"])), aux_affine=aff,
                            aux_mean=mean)
        g.part("mask", pm[0])
        g.ref("temporal data gradient", lambda: g.values("dz"), to_cn(g_pre), BF16)
        g.ref("sum dz", lambda: pm[0].double().sum(dim=1)[:, 0], g_pre.sum(dim=(0, 2, 3)), 1e-4)
        g.ref("sum dz (x - mean)", lambda: pm[0].double().sum(dim=1)[:, 1],
              (g_pre * (c["gx"].double() - c["mean"].double().view(1, -1, 1, 1))).sum(dim=(0, 2, 3)), 1e-4)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ graph convolution
# forward (B, cin, f, T), read-gather kernel sar_graph2_cn8_dispatch: (3, 3, 64, 13) M > 32 -> launch_graph2_cfg<2, 2, 1, 4>, one src
# plane of 3 live lanes; (2, 40, 72, 8) M > 64 -> <2, 2, 2, 2>, 5 src planes (odd), 9 out planes; (2, 64, 24, 6) M <= 32
GRAPH_FWD = [(3, 3, 64, 13), (2, 40, 72, 8), (2, 64, 24, 6)]
# data gradient (B, cin, f, T): M = cin, Kc = f.  (3, 3, 64, 9): M = 3 -> <1, 2, 1, 4>, 5 pad lanes; (2, 40, 72, 9): M = 40 -> <2, 2, 1, 4>,
# 9 src planes; (2, 64, 128, 6): M = 64 is still <2, 2, 1, 4> (the dispatch asks M > 64), so (2, 72, 128, 6) is added for <2, 2, 2, 2>
GRAPH_DGRAD = [(3, 3, 64, 9), (2, 40, 72, 9), (2, 64, 128, 6), (2, 72, 128, 6)]


@functools.lru_cache(maxsize=None)
def graph_fwd_case(B, cin, f, T):
    """tests/test_gpu_cn8.py: test_graph_conv_forward"""
    g = torch.Generator().manual_seed(B * 1000 + cin)
    x = bf16r(B, cin, T, 25, g=g)
    kernel = torch.randn(1, 1, cin, 3 * f, generator=g) * 0.1
    bias = torch.randn(3 * f, generator=g) * 0.1
    ref = graph_ref(x, kernel, bias, _A(), _tables())
    return dict(x=x, bias=bias, ref=ref, pw=_pack(kernel, f, 3 * f, 1, 3, cin, f))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T", GRAPH_FWD)
def test_graph_conv_forward_with_stats(dev, B, cin, f, T, pad):
    """the read-gather kernel, and once more with tables whose g_flags is 0 (conv_graph_cn8_kernel, every gathered tile built by the
    vector ALU): bit for bit the same output and partial sums (test_graph_conv_read_gather_equals_the_unit_builder_bit_for_bit)"""
    from sar_amd import ops8, _lib as L
    c = graph_fwd_case(B, cin, f, T)
    n, ref = B * T * 25, c["ref"]
    assert _tables().g_flags & L.SAR_GRAPH_FEW_DENSE and _tables(False, False).g_flags == 0

    def fn(g):
        for name, tab in (("out", _tables()), ("out (gathering kernel)", _tables(False, False))):
            out = g.out(name, f, n)
            r = ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["x"])), out, c["pw"], B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f, taps=3,
                               bias=c["bias"].to(dev), tables=tab, epi=L.SAR_EPI_STATS)
            g.part("stats " + name, r[0])
        g.ref("graph forward", lambda: g.values("out"), to_cn(ref), BF16)
        g.ref("sum of squares", lambda: g.parts["stats out"].double().sum(dim=1)[:, 1], (ref * ref).sum(dim=(0, 2, 3)), 1e-4)
        g.ref("gathering kernel == read-gather kernel", lambda: g.outs["out (gathering kernel)"][0][:, :n], lambda: g.outs["out"][0][:, :n], 0)
        g.ref("gathering kernel's partial sums", lambda: g.parts["stats out (gathering kernel)"], lambda: g.parts["stats out"], 0)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def graph_dgrad_case(B, cin, f, T):
    """tests/test_gpu_cn8.py: test_graph_conv_data_gradient / test_graph_data_gradient_gated_epilogue"""
    g = torch.Generator().manual_seed(7 * cin + f)
    kernel = torch.randn(1, 1, cin, 3 * f, generator=g) * 0.1
    dout = bf16r(B, f, T, 25, g=g)
    add = bf16r(B, cin, T, 25, g=g)
    u = bf16r(B, cin, T, 25, g=g)
    mean = torch.randn(cin, generator=g) * 0.2
    keep = torch.rand(B, cin, T, 25, generator=g) > 0.4
    kT = kernel[0, 0].view(cin, 3, f).permute(2, 1, 0).reshape(1, 1, f, 3 * cin)      # [m][k*cin + c]
    ref = graph_ref(dout, kT, None, _A().transpose(1, 2), _tables(True))
    return dict(dout=dout, add=add, u=u, mean=mean, keep=keep, ref=ref, pw=_pack(kernel, f, 1, 3 * f, 3, f, cin))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("epi", ["none", "add"])
@pytest.mark.parametrize("B,cin,f,T", GRAPH_DGRAD)
def test_graph_data_gradient(dev, B, cin, f, T, epi, pad):
    """SAR_EPI_NONE and SAR_EPI_ADD; the ADD launch once more on the gathering kernel (g_flags = 0), bit for bit"""
    from sar_amd import ops8, _lib as L
    c = graph_dgrad_case(B, cin, f, T)
    n = B * T * 25
    want = c["ref"] + c["add"].double() if epi == "add" else c["ref"]
    args = dict(B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3)

    def fn(g):
        dx = g.out("dx", cin, n)
        kw = (lambda: dict(epi=L.SAR_EPI_ADD, aux=g.inp(to_cn(c["add"])))) if epi == "add" else (lambda: {})
        ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), dx, c["pw"], tables=_tables(True), **args, **kw())
        g.ref("graph data gradient (%s)" % epi, lambda: g.values("dx"), to_cn(want), BF16)
        if epi == "add":
            dx0 = g.out("dx (gathering kernel)", cin, n)
            ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), dx0, c["pw"], tables=_tables(True, False), **args, **kw())
            g.ref("gathering kernel == read-gather kernel", lambda: dx0[:, :n], lambda: dx[:, :n], 0)
    drive(dev, fn, pad)


def _gated(dev, g, c, B, cin, f, T, pads=(None, None, None, None)):
    """the plain SAR_EPI_ADD launch and the SAR_EPI_ADD_GATE launch with aux, aux2 and the (G, ld_aux2) gate bytes all guarded;
    pads = (out, aux, aux2 and gate bytes, src) override the launch's pad"""
    from sar_amd import ops8, _lib as L
    n = B * T * 25
    args = dict(B=B, V=25, T_src=T, T_out=T, Kc=f, M=cin, taps=3, tables=_tables(True))
    p_out, p_aux, p_aux2, p_src = pads
    plain, gated = g.out("plain", cin, n, p_out), g.out("gated", cin, n, p_out)
    ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"]), p_src), plain, c["pw"], epi=L.SAR_EPI_ADD, aux=g.inp(to_cn(c["add"]), p_aux), **args)
    pm = ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"]), p_src), gated, c["pw"], epi=L.SAR_EPI_ADD_GATE,
                        aux=g.inp(to_cn(c["add"]), p_aux), aux2=g.inp(to_cn(c["u"]), p_aux2),
                        aux_mask=g.mask_in(cn8_mask_bytes(to_cn(c["keep"])), p_aux2), aux_mean=c["mean"].to(dev), **args)
    g.part("gate", pm[0])
    keep = to_cn(c["keep"])
    want = lambda: torch.where(keep, g.values("plain").double(), torch.zeros((), dtype=torch.float64))
    g.ref("gated == ADD gated afterwards", lambda: g.values("gated").double(), want, 0)
    g.ref("plain data gradient", lambda: g.values("plain"), to_cn(c["ref"] + c["add"].double()), BF16)

    def sums():      # test_graph_data_gradient_gated_epilogue's bars: 1e-5 / 2e-5 of the largest absolute row sum
        w = want()
        part = pm[0].cpu().double().sum(dim=1)
        s1, s2 = w.sum(dim=1), (w * (to_cn(c["u"]).double() - c["mean"].double().view(-1, 1))).sum(dim=1)
        scale1 = w.abs().sum(dim=1).max()
        e1, e2 = ((part[:, 0] - s1).abs().max() / scale1).item(), ((part[:, 1] - s2).abs().max() / scale1).item()
        print("gated sums (pad %d): %.2e %.2e" % (g.pad, e1, e2))
        assert e1 <= 1e-5, "sum out (pad %d): %.3e > 1e-5 of the largest absolute row sum" % (g.pad, e1)
        assert e2 <= 2e-5, "sum out (u - mean) (pad %d): %.3e > 2e-5 of the largest absolute row sum" % (g.pad, e2)
        return torch.ones(1)
    g.ref("the gated epilogue's partial sums", sums, torch.ones(1), 0)


@pytest.mark.parametrize("pad", PADS)
def test_graph_data_gradient_gated_epilogue(dev, pad):
    B, cin, f, T = 2, 40, 72, 9
    c = graph_dgrad_case(B, cin, f, T)
    drive(dev, lambda g: _gated(dev, g, c, B, cin, f, T), pad)


def test_graph_data_gradient_gated_epilogue_with_a_different_pad_per_operand(dev):
    """ld_out = n + 1, ld_aux = n + 67, ld_aux2 = n + 5 (the gate bytes share it), ld_src = n + 3: a swapped stride reads a guard"""
    B, cin, f, T = 2, 40, 72, 9
    c = graph_dgrad_case(B, cin, f, T)
    tight, mixed = Launch(dev, 0), Launch(dev, 1)
    _gated(dev, tight, c, B, cin, f, T)
    _gated(dev, mixed, c, B, cin, f, T, pads=(1, 67, 5, 3))
    torch.cuda.synchronize()
    tight.check()
    mixed.check()
    a, b = tight.live(), mixed.live()
    for name in b:
        assert torch.equal(a[name], b[name]), "%s: mixed pads differ from the tight launch" % name


# ------------------------------------------------------------------------------------------------ sar_conv_wgrad_cn8
WGRAD_TEMPORAL = [(2, 64, 13, 1), (2, 64, 14, 2), (2, 72, 11, 1), (2, 40, 12, 2)]


@functools.lru_cache(maxsize=None)
def temporal_wgrad_case(B, f, T, s):
    """tests/test_gpu_cn8.py: test_temporal_conv_weight_gradient"""
    g = torch.Generator().manual_seed(13 * f + T + s)
    x = bf16r(B, f, T, 25, g=g)
    sc = 1 + 0.2 * torch.randn(f, generator=g); sh = 0.3 * torch.randn(f, generator=g)
    To, pad, _ = O.same_pad(T, 9, s)
    du = bf16r(B, f, To, 25, g=g)
    h = bf(torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1))))
    kernel = torch.zeros(9, 1, f, f, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(f, dtype=torch.float64, requires_grad=True)
    gk, gb = torch.autograd.grad(O.temporal_conv(h, kernel, bias, s), (kernel, bias), du.double())
    return dict(x=x, sc=sc, sh=sh, To=To, pad=pad, du=du, gk=gk, gb=gb)


def _temporal_wgrad(dev, B, f, T, s, pad, nsplit=None):
    from sar_amd import ops8, _lib as L
    c = temporal_wgrad_case(B, f, T, s)
    pro = (c["sc"].to(dev), c["sh"].to(dev))

    def fn(g):
        flat = g.flat("dW | dbias", 9 * f * f + f)
        ops8.conv_wgrad(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), g.inp(to_cn(c["du"])), flat, B=B, V=25, T_src=T, T_out=c["To"], Kc=f,
                        M=f, taps=9, stride=s, pad=c["pad"], pro=pro, pro_relu=True, w_stride_tap=f * f, w_stride_c=f, wsize=9 * f * f,
                        bsize=f, nsplit=nsplit)
        g.ref("temporal dW", lambda: flat[:9 * f * f].cpu().view(9, 1, f, f), c["gk"], 1e-5)
        g.ref("temporal dbias", lambda: flat[9 * f * f:], c["gb"], 1e-5)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,f,T,s", WGRAD_TEMPORAL)
def test_temporal_weight_gradient(dev, B, f, T, s, pad):
    _temporal_wgrad(dev, B, f, T, s, pad)


@pytest.mark.parametrize("pad", PADS)
def test_temporal_weight_gradient_with_empty_splits(dev, pad):
    """(2, 64, 13, 1): 2 * ceil(13 / 7) = 4 tiles, nsplit = 7: three splits have no tile and must write zeros to their slabs"""
    from sar_amd import _lib as L
    assert 2 * -(-13 // L.load().sar_conv_wgrad_cn8_tile_frames(L.SAR_CONV_TEMPORAL)) < 7
    _temporal_wgrad(dev, 2, 64, 13, 1, pad, nsplit=7)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T,s", RESIDUAL)
def test_residual_weight_gradient(dev, B, cin, f, T, s, pad):
    from sar_amd import ops8, _lib as L
    c = residual_case(B, cin, f, T, s)

    def fn(g):
        flat = g.flat("dW | dbias", cin * f + f)
        ops8.conv_wgrad(L.SAR_CONV_TEMPORAL, g.inp(to_cn(c["x"])), g.inp(to_cn(c["dr"])), flat, B=B, V=25, T_src=T, T_out=c["To"], Kc=cin,
                        M=f, taps=1, stride=s, pad=0, w_stride_tap=0, w_stride_c=f, wsize=cin * f, bsize=f)
        g.ref("residual dW", lambda: flat[:cin * f].cpu().view(1, 1, cin, f), c["gk"], 1e-5)
        g.ref("residual dbias", lambda: flat[cin * f:], c["gb"], 1e-5)
    drive(dev, fn, pad)


@functools.lru_cache(maxsize=None)
def graph_wgrad_case(B, cin, f, T):
    """tests/test_gpu_cn8.py: test_graph_conv_weight_gradient"""
    g = torch.Generator().manual_seed(17 * cin + f)
    x = bf16r(B, cin, T, 25, g=g)
    dg = bf16r(B, f, T, 25, g=g)
    tab = _tables()
    idx, wt = tab.idx.cpu(), tab.wt.cpu()
    gk = torch.zeros(cin, 3 * f, dtype=torch.float64)
    gb = torch.zeros(3 * f, dtype=torch.float64)
    A = _A()
    for k in range(3):
        z = torch.zeros(B, cin, T, 25)
        for w in range(25):
            acc = wt[k, w, 0] * x[:, :, :, idx[k, w, 0]]
            for j in range(1, tab.nz[k]):
                acc = torch.addcmul(acc, x[:, :, :, idx[k, w, j]], wt[k, w, j])
            z[:, :, :, w] = acc
        gk[:, k * f:(k + 1) * f] = torch.einsum("bctv,bmtv->cm", bf(z), dg.double())
        gb[k * f:(k + 1) * f] = torch.einsum("bmtv,v->m", dg.double(), A[k].double().sum(dim=0))
    return dict(x=x, dg=dg, gk=gk, gb=gb)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("B,cin,f,T", [(3, 3, 64, 9), (2, 40, 72, 9)])
def test_graph_weight_gradient(dev, B, cin, f, T, pad):
    """with slice0_identity on and off: bit equal"""
    from sar_amd import ops8, _lib as L
    c = graph_wgrad_case(B, cin, f, T)
    wsize, bsize = cin * 3 * f, 3 * f
    assert _tables().slice0_identity and not _tables_general_slice0().slice0_identity

    def fn(g):
        flats = []
        for name, tab in (("dW | dbias", _tables()), ("dW | dbias (general slice 0)", _tables_general_slice0())):
            flat = g.flat(name, wsize + bsize)
            ops8.conv_wgrad(L.SAR_CONV_GRAPH, g.inp(to_cn(c["x"])), g.inp(to_cn(c["dg"])), flat, B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f,
                            taps=3, tables=tab, w_stride_tap=f, w_stride_c=3 * f, wsize=wsize, bsize=bsize)
            flats.append(flat)
        g.ref("graph dW", lambda: flats[0][:wsize].cpu().view(cin, 3 * f), c["gk"], 1e-5)
        g.ref("graph dbias", lambda: flats[0][wsize:], c["gb"], 1e-5)
        g.ref("slice-0 shortcut == general path", flats[1], flats[0], 0)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ element-wise
# (C, n): (20, 777) 3 planes with 4 pad lanes, n odd and < one EW_U pass of 1024; (64, 350) full planes; (8, 1031) one plane, n one
# pass of 256 x EW_U units plus 7: the second grid-stride block of the streaming kernels holds 7 live units
TAIL_SHAPES = [(20, 777), (64, 350), (8, 1031)]


@functools.lru_cache(maxsize=None)
def tail_case(C, n):
    """tests/test_gpu_cn8.py: test_block_tail_forward_backward / test_block_tail_relu_mask_is_bit_identical"""
    g = torch.Generator().manual_seed(C + n)
    rnd = lambda *s: torch.randn(*s, generator=g)
    u, r, dy = bf16r(C, n, g=g), bf16r(C, n, g=g), bf16r(C, n, g=g)
    sc, sh, rsc, rsh = 1 + 0.2 * rnd(C), 0.3 * rnd(C), 1 + 0.2 * rnd(C), 0.3 * rnd(C)
    k, rk = [0.5 * rnd(C) for _ in range(3)], [0.5 * rnd(C) for _ in range(3)]
    mu, mr = 0.1 * rnd(C), 0.1 * rnd(C)
    col = lambda t: t.double().view(-1, 1)
    z = u.double() * col(sc) + col(sh)
    y = {0: torch.relu(z), 1: torch.relu(z + r.double()), 2: torch.relu(z + r.double() * col(rsc) + col(rsh))}
    ystored = y[2].float().bfloat16().float()        # a stored y for the backward passes (inputs there)
    return dict(u=u, r=r, dy=dy, sc=sc, sh=sh, rsc=rsc, rsh=rsh, k=k, rk=rk, mu=mu, mr=mr, y=y, ystored=ystored, col=col)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_forward(dev, C, n, kind, pad):
    """sar_bn_add_relu_fwd_cn8 without and with a mask: bit-equal outputs, the mask equal to its definition on the stored y"""
    from sar_amd import ops8
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    rs = (d(c["rsc"]), d(c["rsh"])) if kind == 2 else (None, None)

    def fn(g):
        u, r = g.inp(c["u"]), (g.inp(c["r"]) if kind else None)
        y0, y1, mask = g.out("y", C, n), g.out("y (masked kernel)", C, n), g.mask_out("relu", C, n)
        ops8.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), kind, r, rs[0], rs[1], y0, C, n=n)
        ops8.bn_add_relu_fwd(u, d(c["sc"]), d(c["sh"]), kind, r, rs[0], rs[1], y1, C, mask=mask, n=n)
        g.ref("block tail forward", lambda: g.values("y"), c["y"][kind], BF16)
        g.ref("masked kernel == plain kernel", lambda: y1[:, :n], lambda: y0[:, :n], 0)
        g.ref("mask == its definition", lambda: mask[:, :n], lambda: cn8_mask_bytes(g.values("y") > 0), 0)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_backward_reduce(dev, C, n, pad):
    """sar_bn_add_relu_bwd_reduce_cn8, plain, with a mask and with a tail: partials (sum dz, sum dz (u - mu), sum dz (r - mr)), dz = dy where the
    stored y > 0.  The folded finalisation against sar_bn_bwd_finalize_f32 on the plain partials: the same sums in another order, 1e-6
    (tests/test_gpu_guard_bands.py's bar for it); the ticket array is back to zero."""
    from sar_amd import ops, ops8
    from sar_amd.stgcn import _BN
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    ys = c["ystored"]
    dz = c["dy"].double() * (ys > 0)
    sums = [dz.sum(1), (dz * (c["u"].double() - c["col"](c["mu"]))).sum(1), (dz * (c["r"].double() - c["col"](c["mr"]))).sum(1)]
    gam, rgam = 1 + 0.2 * torch.sin(torch.arange(C, dtype=torch.float32)), 1 + 0.2 * torch.cos(torch.arange(C, dtype=torch.float32))
    rstd = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(C))

    def fn(g):
        dy, y, u, r = g.inp(c["dy"]), g.inp(ys), g.inp(c["u"]), g.inp(c["r"])
        p0, n0 = ops8.bn_add_relu_bwd_reduce(dy, y, u, r, C, d(c["mu"]), d(c["mr"]), n=n)
        assert n0 == max(1, -(-n // 8192))          # sized from the live width, not from ld
        g.part("plain", p0, 3)
        for j, name in enumerate(("sum dz", "sum dz (u - mu)", "sum dz (r - mr)")):
            g.ref(name, lambda j=j: p0.double().sum(dim=1)[:, j], sums[j], 1e-4)
        p1, n1 = ops8.bn_add_relu_bwd_reduce(dy, None, u, r, C, d(c["mu"]), d(c["mr"]), mask=g.mask_in(cn8_mask_bytes(ys > 0)), n=n)
        assert n1 == n0
        g.part("masked", p1, 3)
        g.ref("masked partials == plain partials", lambda: p1[:, :, :3], lambda: p0[:, :, :3], 0)
        z = lambda: torch.zeros(C, device=dev)
        gamd, rgamd = d(gam), d(rgam)      # (sar_bn_tail holds raw pointers: the tensors must outlive the launch)
        bn, rbn, bn0, rbn0 = _BN(C, dev), _BN(C, dev), _BN(C, dev), _BN(C, dev)
        for b in (bn, rbn, bn0, rbn0):
            b.rstd.copy_(d(rstd))
        dg0, db0, rdg0, rdb0, dg, db, rdg, rdb = z(), z(), z(), z(), z(), z(), z(), z()
        ops.bn_bwd_finalize(p0, n0, n0 * 4, 4, 0, 1, C, n, gamd, d(c["mu"]), bn0.rstd, dg0, db0, bn0.k1, bn0.k2, bn0.k3)
        ops.bn_bwd_finalize(p0, n0, n0 * 4, 4, 0, 2, C, n, rgamd, d(c["mr"]), rbn0.rstd, rdg0, rdb0, rbn0.k1, rbn0.k2, rbn0.k3)
        tail = ops.make_bn_tail(dev, n, gamd, bn, dg, db, rgamd, rbn, rdg, rdb)
        p2, _ = ops8.bn_add_relu_bwd_reduce(dy, y, u, r, C, d(c["mu"]), d(c["mr"]), tail=tail, n=n)
        g.part("tail", p2, 3)
        g.ref("tail partials == plain partials", lambda: p2[:, :, :3], lambda: p0[:, :, :3], 0)
        for name, got, want in [("dgamma", dg, dg0), ("dbeta", db, db0), ("k1", bn.k1, bn0.k1), ("k2", bn.k2, bn0.k2), ("k3", bn.k3, bn0.k3),
                                ("rdgamma", rdg, rdg0), ("rdbeta", rdb, rdb0), ("rk1", rbn.k1, rbn0.k1), ("rk2", rbn.k2, rbn0.k2),
                                ("rk3", rbn.k3, rbn0.k3)]:
            g.part("tail " + name, got)
            g.ref("folded finalisation " + name, got, want, 1e-6)
        g.keep = (gamd, rgamd, bn, rbn, tail)
        g.ref("ticket array back to zero", lambda: ops.bn_tail_tickets(dev).abs().sum().reshape(1).float(), torch.zeros(1), 0)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C,n", TAIL_SHAPES)
def test_block_tail_backward_apply_and_affine2(dev, C, n, pad):
    """sar_bn_add_relu_bwd_apply_cn8 without / with a mask: du = k1 dz + k2 u + k3, dr = rk1 dz + rk2 r + rk3, dz_out = dz (bitwise: a copy
    or a zero); sar_affine2_cn8: out = k1 a + k2 b + k3"""
    from sar_amd import ops8
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    ys = c["ystored"]
    dz = c["dy"].double() * (ys > 0)
    col, D = c["col"], lambda t: t.double()
    k, rk = c["k"], c["rk"]
    kd, rkd = [d(v) for v in k], [d(v) for v in rk]

    def fn(g):
        dy, y, u, r = g.inp(c["dy"]), g.inp(ys), g.inp(c["u"]), g.inp(c["r"])
        du, dr, dzo, aff = g.out("du", C, n), g.out("dr", C, n), g.out("dz", C, n), g.out("affine2", C, n)
        ops8.bn_add_relu_bwd_apply(dy, y, u, r, kd, rkd, du, dr, dzo, C, n=n)
        ops8.affine2(dy, u, kd, aff, C, n=n)
        g.ref("du", lambda: g.values("du"), col(k[0]) * dz + col(k[1]) * D(c["u"]) + col(k[2]), BF16)
        g.ref("dr", lambda: g.values("dr"), col(rk[0]) * dz + col(rk[1]) * D(c["r"]) + col(rk[2]), BF16)
        g.ref("dz_out", lambda: g.values("dz").double(), dz, 0)
        g.ref("affine2", lambda: g.values("affine2"), col(k[0]) * D(c["dy"]) + col(k[1]) * D(c["u"]) + col(k[2]), BF16)
        du1, dr1, dz1 = g.out("du (mask)", C, n), g.out("dr (mask)", C, n), g.out("dz (mask)", C, n)
        ops8.bn_add_relu_bwd_apply(dy, None, u, r, kd, rkd, du1, dr1, dz1, C, mask=g.mask_in(cn8_mask_bytes(ys > 0)), n=n)
        for a, b, name in ((du1, du, "du"), (dr1, dr, "dr"), (dz1, dzo, "dz")):
            g.ref("masked %s == plain" % name, lambda a=a: a[:, :n], lambda b=b: b[:, :n], 0)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ data_bn, pool, layout conversion
@functools.lru_cache(maxsize=None)
def data_bn_case():
    """tests/test_gpu_cn8.py: test_pooling_and_data_bn at N, T, M = 3, 9, 2"""
    from sar_amd.bone import NTU_BONE_PAIRS
    g = torch.Generator().manual_seed(3)
    N, T, M = 3, 9, 2
    x = 0.3 * torch.randn(N, 3, T, 25, M, generator=g)
    bp = np.full(25, -1, dtype=np.int32)
    for v1, v2 in NTU_BONE_PAIRS:
        bp[v1 - 1] = v2 - 1
    scale, shift = 1 + 0.1 * torch.randn(75, generator=g), 0.1 * torch.randn(75, generator=g)
    dy = bf16r(3, N * M * T * 25, g=g)
    mean = 0.05 * torch.randn(75, generator=g)
    return dict(x=x, bone=torch.from_numpy(bp), scale=scale, shift=shift, dy=dy, mean=mean)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("bone", [False, True], ids=["joints", "bones"])
def test_data_bn_apply_and_backward_reduce(dev, bone, pad):
    """identical values (rounded) to the fp32 kernel, incl. the fused bone transform; the backward partials bit for bit"""
    from sar_amd import ops, ops8
    c = data_bn_case()
    N, _, T, _, M = c["x"].shape
    n = N * M * T * 25
    x, parent = c["x"].to(dev), (c["bone"].to(dev) if bone else None)
    scale, shift, mean = c["scale"].to(dev), c["shift"].to(dev), c["mean"].to(dev)
    h32, p32 = torch.empty((3, n), device=dev), torch.empty((75, N, 2), device=dev)
    ops.data_bn_apply(x, parent, scale, shift, h32)
    ops.data_bn_bwd_reduce(x, parent, c["dy"].to(dev), mean, p32)

    def fn(g):
        h8 = g.out("h", 3, n)
        ops8.data_bn_apply(x, parent, scale, shift, h8)
        p8 = torch.empty((75, N, 2), device=dev)
        ops8.data_bn_bwd_reduce(x, parent, g.inp(c["dy"]), mean, p8)
        g.part("backward", p8)
        g.ref("data_bn == the fp32 kernel rounded", lambda: g.values("h"), lambda: h32.bfloat16().float(), 0)
        g.ref("backward partials == the fp32 kernel's", p8, p32, 0)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
def test_pool_forward_and_backward(dev, pad):
    from sar_amd import ops8
    g0 = torch.Generator().manual_seed(3)
    C, B, TV, Mp = 40, 6, 75, 2
    y = bf16r(C, B * TV, g=g0)
    dfeat = torch.randn(B // Mp, C, generator=g0)
    ref = y.double().view(C, B // Mp, Mp * TV).mean(dim=2).t()
    dref = (dfeat.double().t() / (Mp * TV)).view(C, B // Mp, 1).expand(C, B // Mp, Mp * TV).reshape(C, -1)

    def fn(g):
        feat, dy = g.flat("feat", (B // Mp) * C), g.out("dy", C, B * TV)
        ops8.pool_fwd(g.inp(y), C, B, TV, Mp, feat.view(B // Mp, C))
        ops8.pool_bwd(dfeat.to(dev), C, B, TV, Mp, dy)
        g.ref("pooled features", lambda: feat.view(B // Mp, C), ref, 1e-5)
        g.ref("pool backward", lambda: g.values("dy"), dref, BF16)
    drive(dev, fn, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C", [3, 20, 64])
def test_layout_conversion(dev, C, pad):
    """sar_cn_to_cn8 / sar_cn8_to_cn: the fp32 side guarded by guarded() (ld_x = n + pad floats), the CN8 side by guarded_cn8: exact
    copies of bf16-representable values, by the layout's definition"""
    from sar_amd import ops8
    n = 333
    x = bf16r(C, n, g=torch.Generator().manual_seed(C))

    def fn(g):
        x8 = g.out("x8", C, n)
        ops8.from_cn(guarded(x, g.pad, NAN, dev, 4, 2)[0], out=x8)
        back = g.rows_out("back", C, n)
        ops8.to_cn(g.inp(x), C, n=n, out=back)
        g.ref("cn -> cn8", lambda: g.values("x8"), x, 0)
        g.ref("cn8 -> cn", back, x, 0)
    drive(dev, fn, pad)


# ------------------------------------------------------------------------------------------------ 6: ld below the live width
@pytest.mark.parametrize("short", ["ld_src", "ld_out", "ld_aux"])
def test_conv_gemm_rejects_a_leading_dimension_below_the_live_width(dev, short):
    from sar_amd import ops8, _lib as L
    B, f, T, s = 2, 64, 13, 1
    c = temporal_dgrad_case(B, f, T, s)
    n = B * T * 25
    cut = lambda name: n - 1 if short == name else n

    def fn(g):
        src = g.inp(to_cn(c["du"])[:, :cut("ld_src")])
        aux = g.inp(to_cn(c["gx"])[:, :cut("ld_aux")])
        ops8.conv_gemm(L.SAR_CONV_TEMPORAL, src, g.out("dz", f, cut("ld_out")), c["pw"], B=B, V=25, T_src=c["To"], T_out=T, Kc=f, M=f,
                       taps=9, stride=s, pad=c["pad"], transposed=True, epi=L.SAR_EPI_ADD, aux=aux)
    rejected(dev, fn)


def test_graph_gate_rejects_ld_aux2_below_the_live_width(dev):
    B, cin, f, T = 2, 40, 72, 9
    c = graph_dgrad_case(B, cin, f, T)

    def fn(g):
        from sar_amd import ops8, _lib as L
        n = B * T * 25
        ops8.conv_gemm(L.SAR_CONV_GRAPH, g.inp(to_cn(c["dout"])), g.out("gated", cin, n), c["pw"], epi=L.SAR_EPI_ADD_GATE,
                       aux=g.inp(to_cn(c["add"])), aux2=g.inp(to_cn(c["u"])[:, :n - 1]),
                       aux_mask=g.mask_in(cn8_mask_bytes(to_cn(c["keep"]))[:, :n - 1]), aux_mean=c["mean"].to(dev), B=B, V=25, T_src=T,
                       T_out=T, Kc=f, M=cin, taps=3, tables=_tables(True))
    rejected(dev, fn)


@pytest.mark.parametrize("short", ["ld_src", "ld_dout"])
def test_conv_wgrad_rejects_a_leading_dimension_below_the_live_width(dev, short):
    from sar_amd import ops8, _lib as L
    B, f, T, s = 2, 64, 13, 1
    c = temporal_wgrad_case(B, f, T, s)
    n = B * T * 25

    def fn(g):
        src = g.inp(to_cn(c["x"])[:, :n - 1 if short == "ld_src" else n])
        dout = g.inp(to_cn(c["du"])[:, :n - 1 if short == "ld_dout" else n])
        ops8.conv_wgrad(L.SAR_CONV_TEMPORAL, src, dout, g.flat("dW | dbias", 9 * f * f + f), B=B, V=25, T_src=T, T_out=c["To"], Kc=f, M=f,
                        taps=9, stride=s, pad=c["pad"], w_stride_tap=f * f, w_stride_c=f, wsize=9 * f * f, bsize=f)
    rejected(dev, fn)


@pytest.mark.parametrize("which", ["fwd", "fwd_mask", "bwd_reduce", "bwd_reduce_mask", "bwd_reduce_tail", "bwd_apply", "bwd_apply_mask",
                                   "affine2"])
def test_elementwise_rejects_a_leading_dimension_below_the_live_width(dev, which):
    """tensors of ld = n - 1 units per plane with the live width n"""
    from sar_amd import ops, ops8
    from sar_amd.stgcn import _BN
    C, n = 20, 777
    c = tail_case(C, n)
    d = lambda t: t.to(dev)
    kd = [d(v) for v in c["k"]]

    def fn(g):
        i = lambda t: g.inp(t[:, :n - 1])
        o = lambda name: g.out(name, C, n - 1)
        mb = cn8_mask_bytes(c["ystored"] > 0)[:, :n - 1]
        if which == "fwd":
            ops8.bn_add_relu_fwd(i(c["u"]), d(c["sc"]), d(c["sh"]), 1, i(c["r"]), None, None, o("y"), C, n=n)
        elif which == "fwd_mask":
            ops8.bn_add_relu_fwd(i(c["u"]), d(c["sc"]), d(c["sh"]), 1, i(c["r"]), None, None, o("y"), C, mask=g.mask_out("relu", C, n - 1), n=n)
        elif which == "bwd_reduce":
            ops8.bn_add_relu_bwd_reduce(i(c["dy"]), i(c["ystored"]), i(c["u"]), i(c["r"]), C, d(c["mu"]), d(c["mr"]), n=n)
        elif which == "bwd_reduce_mask":
            ops8.bn_add_relu_bwd_reduce(i(c["dy"]), None, i(c["u"]), i(c["r"]), C, d(c["mu"]), d(c["mr"]), mask=g.mask_in(mb), n=n)
        elif which == "bwd_reduce_tail":
            z = lambda: torch.zeros(C, device=dev)
            g.keep = (z(), z(), z(), z(), z(), z(), _BN(C, dev), _BN(C, dev))
            tail = ops.make_bn_tail(dev, n, g.keep[0], g.keep[6], g.keep[1], g.keep[2], g.keep[3], g.keep[7], g.keep[4], g.keep[5])
            ops8.bn_add_relu_bwd_reduce(i(c["dy"]), i(c["ystored"]), i(c["u"]), i(c["r"]), C, d(c["mu"]), d(c["mr"]), tail=tail, n=n)
        elif which == "bwd_apply":
            ops8.bn_add_relu_bwd_apply(i(c["dy"]), i(c["ystored"]), i(c["u"]), i(c["r"]), kd, kd, o("du"), o("dr"), o("dz"), C, n=n)
        elif which == "bwd_apply_mask":
            ops8.bn_add_relu_bwd_apply(i(c["dy"]), None, i(c["u"]), i(c["r"]), kd, kd, o("du"), o("dr"), o("dz"), C, mask=g.mask_in(mb), n=n)
        else:
            ops8.affine2(i(c["dy"]), i(c["u"]), kd, o("affine2"), C, n=n)
    rejected(dev, fn)


@pytest.mark.parametrize("which", ["data_bn_apply", "data_bn_bwd_reduce", "pool_fwd", "pool_bwd", "cn_to_cn8", "cn8_to_cn"])
def test_data_bn_pool_and_conversion_reject_a_leading_dimension_below_the_live_width(dev, which):
    from sar_amd import ops8
    c = data_bn_case()
    N, _, T, _, M = c["x"].shape
    n = N * M * T * 25
    C, B, TV, Mp = 40, 6, 75, 2
    x = bf16r(C, B * TV, g=torch.Generator().manual_seed(1))

    def fn(g):
        if which == "data_bn_apply":
            ops8.data_bn_apply(c["x"].to(dev), None, c["scale"].to(dev), c["shift"].to(dev), g.out("h", 3, n - 1))
        elif which == "data_bn_bwd_reduce":
            ops8.data_bn_bwd_reduce(c["x"].to(dev), None, g.inp(c["dy"][:, :n - 1]), c["mean"].to(dev), g.flat("partials", 75 * N * 2))
        elif which == "pool_fwd":
            ops8.pool_fwd(g.inp(x[:, :B * TV - 1]), C, B, TV, Mp, g.flat("feat", (B // Mp) * C))
        elif which == "pool_bwd":
            ops8.pool_bwd(torch.zeros(B // Mp, C, device=dev), C, B, TV, Mp, g.out("dy", C, B * TV - 1))
        elif which == "cn_to_cn8":
            ops8.from_cn(x.to(dev), out=g.out("x8", C, B * TV - 1))
        else:
            back = g.rows_out("back", C, B * TV)
            ops8.to_cn(g.inp(x[:, :B * TV - 1]), C, n=B * TV, out=back)
    rejected(dev, fn)


# ------------------------------------------------------------------------------------------------ the non-default staging paths
CONV_CASES = "temporal_conv or residual_conv or graph_conv or graph_data_gradient"
CHILD_TIMEOUT = 90      # measured: 5 s per child, most of it interpreter start-up and the float64 references


def _child_pytest(env, select):
    """cases of this file in a fresh interpreter (the switches are read once per process), as tests/test_gpu_lds_overlays.py:
    _pytest_with_lib"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "(%s) and not staging" % select], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT, cwd=ROOT)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (tail, r.stderr[-1500:])


def test_register_staging_and_the_gathering_graph_kernel(dev):
    """SAR_CN8_DMA=0: the 9-tap data gradients with M > 32 on the register-staged conv_gemm_cn8_kernel<1 / 3, 9, 2, 2, 1, 4>;
    SAR_GRAPH_READ_GATHER=0: every graph launch on conv_graph_cn8_kernel, with the matrix-core adjacency gather where the tables
    allow it (the gated epilogue exists in the read-gather kernel only and is not selected)"""
    _child_pytest(dict(SAR_CN8_DMA="0", SAR_GRAPH_READ_GATHER="0"), "(%s) and not gated" % CONV_CASES)


def test_deep_prefetch_staging(dev):
    """SAR_CN8_DMA=0 SAR_CN8_DB=1: conv_gemm_cn8_db_kernel for the 9-tap stride-1 forward and the stride-1 / parity-split data
    gradients with M > 32 (the switch reaches no graph and no 1-tap launch: the 9-tap cases only)"""
    _child_pytest(dict(SAR_CN8_DMA="0", SAR_CN8_DB="1"), "temporal_conv")
