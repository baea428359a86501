"""GPU parity of the 2-D convolution kernels (forward, data gradient, weight gradient) at every layer shape of the
reference's ResNet-18 (models/resnet18.py) against torch CPU float64 convolutions; max-pool stem tail; Adam.

The test_rect_* / test_stem_data_gradient_* tests run the groups A to G of tests/conv2d_rect_cases.py: rectangular and odd-sized images,
the paths no square shape reaches.  Worst error per group over its cases and both arithmetics, MEASURED on an MI355X (bars: 2e-5 for
tensors and the sum of squares, 1e-4 for the centred partial sums):
  A  stride-2 data gradient    dz 3.8e-7, sum dz 2.6e-7, sum dz (aux - mean) 2.1e-7, with the compact aux 3.0e-7
  B  1x1 / stride 2            y 1.4e-7, sum y^2 7.7e-8, dW 1.6e-7, dx 1.8e-7
  C  stem 7x7                  y 3.1e-7, sum y^2 4.3e-8, dW 3.9e-7
  D  stem data gradient        dx 1.2e-6
  E  bn + relu + max-pool      y 4.7e-8, dz 1.3e-7, sum dz 1.1e-7, sum dz (x - mean) 1.4e-7
  F  3x3 weight gradient       dW 3.0e-7 (v0..v6 with a ragged last row tile, and the generic loop)
  G  several images per tile   y 4.5e-7, sum y^2 9.9e-8, dz 9.0e-7, sum dz 4.1e-7, sum dz (aux - mean) 3.4e-7"""
import pytest
import torch
import torch.nn.functional as F

import conv2d_rect_cases as RC
from util import rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5

# (cin, cout, k, stride, H)   -- square images; all conv shapes of resnet18(num_filters=64) on 256x256 inputs
SHAPES = [(1, 64, 7, 2, 256), (64, 64, 3, 1, 64), (64, 128, 3, 2, 64), (64, 128, 1, 2, 64), (128, 128, 3, 1, 32),
          (128, 256, 3, 2, 32), (128, 256, 1, 2, 32), (256, 256, 3, 1, 16), (256, 512, 3, 2, 16), (256, 512, 1, 2, 16),
          (512, 512, 3, 1, 8), (16, 32, 3, 2, 64), (8, 8, 3, 1, 16), (24, 40, 3, 1, 20)]


def cn(x):     # (B,C,H,W) -> [C][B*H*W]
    B, C, H, W = x.shape
    return x.permute(1, 0, 2, 3).reshape(C, B * H * W).contiguous()


def uncn(y, B, H, W):
    return y.reshape(y.shape[0], B, H, W).permute(1, 0, 2, 3)


@pytest.mark.parametrize("cin,cout,k,s,H", SHAPES)
def test_conv2d_forward_dgrad_wgrad(cin, cout, k, s, H):
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    B, pad, taps = 2, k // 2, k * k
    g = torch.Generator().manual_seed(cin * 7 + cout + k + s)
    x = torch.randn(B, cin, H, H, generator=g).double().requires_grad_(True)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * taps) ** 0.5).double().requires_grad_(True)
    sc = (1 + 0.2 * torch.randn(cin, generator=g)).double()
    sh = (0.3 * torch.randn(cin, generator=g)).double()
    use_pro = cin > 1
    pre = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) if use_pro else x
    hin = torch.relu(pre) if use_pro else x
    y = F.conv2d(hin, w, None, stride=s, padding=pad)
    Ho = y.shape[2]
    dy = torch.randn(y.shape, generator=g)
    gh, gw = torch.autograd.grad(y, (hin if use_pro else x, w), dy.double())
    geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=H, H_out=Ho, W_out=Ho, KH=k, KW=k, stride=s, pad=pad)
    wd = w.detach().float().to(dev).contiguous()
    wf = torch.empty(taps * cin * cout, device=dev)
    ops.permute3(wd, wf, taps, cin, cout, 1, taps, cin * taps)
    xd, dyd = cn(x.detach().float()).to(dev), cn(dy).to(dev)
    pro = (sc.float().to(dev), sh.float().to(dev)) if use_pro else None
    # forward (+ BN statistics)
    out = torch.empty((cout, B * Ho * Ho), device=dev)
    r = ops.conv2d_gemm(xd, out, wf, cin * cout, cout, epi=L.SAR_EPI_STATS, pro=pro, pro_relu=use_pro, **geo)
    torch.cuda.synchronize()
    assert rel_err(uncn(out.cpu(), B, Ho, Ho), y) < TOL
    part = r[0].cpu().double().sum(1)
    assert rel_err(part[:, 1], (y * y).sum(dim=(0, 2, 3))) < TOL
    # weight gradient
    tmp = torch.empty(taps * cin * cout, device=dev)
    ops.conv2d_wgrad(xd, dyd, tmp, pro=pro, pro_relu=use_pro, **geo)
    gwd = torch.empty((cout, cin, k, k), device=dev)
    ops.permute3(tmp, gwd, cout, cin, taps, 1, cout, cin * cout)
    torch.cuda.synchronize()
    assert rel_err(gwd.cpu(), gw) < TOL
    # data gradient (not needed for the 1-channel stem)
    if cin > 1:
        wb = torch.empty(taps * cin * cout, device=dev)
        ops.permute3(wd, wb, taps, cout, cin, 1, cin * taps, taps)
        dx = torch.empty((cin, B * H * H), device=dev)
        add = torch.randn(cin, B * H * H, generator=g)
        ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=add.to(dev), B=B, Kc=cout, M=cin, H_src=Ho,
                        W_src=Ho, H_out=H, W_out=H, KH=k, KW=k, stride=s, pad=pad, transposed=True)
        torch.cuda.synchronize()
        assert rel_err(uncn(dx.cpu() - add, B, H, H), gh) < TOL


@pytest.mark.parametrize("cin,cout,H", [(64, 128, 64), (256, 512, 16), (16, 32, 12), (8, 16, 15)])
def test_stride2_data_gradient_parity_classes(cin, cout, H):
    """3x3 / stride 2 / pad 1 data gradient: the parity-class launches (H even; H = 15 takes the masked kernel) with (a) the
    ReLU-mask epilogue + BatchNorm partial sums spread over the four launches, (b) SAR_C2D_AUX_EVEN_PIXELS: the compact data
    gradient of the parallel 1x1 / stride 2 convolution (models/resnet18.py:92-100) added at the even pixels."""
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    B, k, s, pad = 3, 3, 2, 1
    g = torch.Generator().manual_seed(cin + H)
    x = torch.randn(B, cin, H, H, generator=g).double().requires_grad_(True)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).double()
    y = F.conv2d(x, w, None, stride=2, padding=1)
    Ho = y.shape[2]
    dy = torch.randn(y.shape, generator=g)
    gx, = torch.autograd.grad(y, x, dy.double())
    wb = torch.empty(9 * cin * cout, device=dev)
    ops.permute3(w.float().to(dev).contiguous(), wb, 9, cout, cin, 1, cin * 9, 9)
    dyd = cn(dy).to(dev)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Ho, H_out=H, W_out=H, KH=3, KW=3, stride=2, pad=1, transposed=True)
    # (a) MASK: dz = dx where relu'(aux * sc + sh); partials = (sum dz, sum dz (aux - mean))
    aux = torch.randn(cin, B * H * H, generator=g)
    sc, sh, mu = 1 + 0.2 * torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    dx = torch.empty((cin, B * H * H), device=dev)
    r = ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=aux.to(dev), aux_affine=(sc.to(dev), sh.to(dev)),
                        aux_mean=mu.to(dev), **geo)
    torch.cuda.synchronize()
    mask = (aux.double() * sc.double()[:, None] + sh.double()[:, None]) > 0
    ref = cn(gx) * mask
    assert rel_err(dx.cpu(), ref) < TOL
    part = r[0].cpu().double().sum(1)
    assert rel_err(part[:, 0], ref.sum(1)) < 1e-4 and rel_err(part[:, 1], (ref * (aux.double() - mu.double()[:, None])).sum(1)) < 1e-4
    # (b) compact aux at the even pixels
    if H % 2 == 0:
        small = torch.randn(cin, B * Ho * Ho, generator=g)
        dx2 = torch.empty((cin, B * H * H), device=dev)
        ops.conv2d_gemm(dyd, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=small.to(dev), aux_even_pixels=True, **geo)
        torch.cuda.synchronize()
        full = torch.zeros(B, cin, H, H, dtype=torch.float64)
        full[:, :, ::2, ::2] = uncn(small.double(), B, Ho, Ho)
        assert rel_err(uncn(dx2.cpu(), B, H, H), gx + full) < TOL
    else:
        with pytest.raises(L.SarError):
            ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=aux.to(dev), aux_even_pixels=True, **geo)


def test_stem_tail_maxpool_forward_backward():
    from sar_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    B, C, H = 2, 8, 30
    x = torch.randn(B, C, H, H, generator=g).double().requires_grad_(True)
    sc = (1 + 0.2 * torch.randn(C, generator=g)).double()
    sh = (0.3 * torch.randn(C, generator=g)).double()
    a = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    y = F.max_pool2d(a, 3, 2, 1)
    Ho = y.shape[2]
    dy = torch.randn(y.shape, generator=g)
    (gx,) = torch.autograd.grad(y, x, dy.double())
    gz = gx / sc.view(1, -1, 1, 1)                       # gradient w.r.t. the BN output
    xd = cn(x.detach().float()).to(dev)
    yd = torch.empty((C, B * Ho * Ho), device=dev)
    scd, shd = sc.float().to(dev), sh.float().to(dev)
    ops.bn_relu_maxpool_fwd(xd, scd, shd, yd, B, H, H)
    dz = torch.empty_like(xd)
    mean = x.detach().mean(dim=(0, 2, 3)).float().to(dev)
    part, nparts = ops.bn_relu_maxpool_bwd(xd, scd, shd, mean, cn(dy).to(dev), dz, B, H, H)
    torch.cuda.synchronize()
    assert rel_err(uncn(yd.cpu(), B, Ho, Ho), y) < TOL
    assert rel_err(uncn(dz.cpu(), B, H, H), gz) < TOL
    ps = part.cpu().double().sum(1)
    assert rel_err(ps[:, 0], gz.sum(dim=(0, 2, 3))) < 1e-4
    assert rel_err(ps[:, 1], (gz * (x.detach() - x.detach().mean(dim=(0, 2, 3), keepdim=True))).sum(dim=(0, 2, 3))) < 1e-4


# ------------------------------------------------------------------------------------------------ rectangular and odd-sized images
# tests/conv2d_rect_cases.py holds the tables and the float64 references; tests/test_conv2d_rect_cases.py (CPU) shows that an H / W
# exchange moves every reference by more than 1e-2 and which host path each case takes.  Each test prints its figures before it asserts.
def _said(group, case, **errs):
    print("RECT %s %s %s" % (group, case, " ".join("%s=%.2e" % kv for kv in errs.items())))
    return errs


def _rect_conv(group, cin, cout, k, s, H, W, B, forward=True, wgrad=True, dgrad=True):
    """test_conv2d_forward_dgrad_wgrad on an H x W image: forward with STATS, weight gradient, data gradient with the ADD epilogue"""
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    c = RC.conv_ref(cin, cout, k, s, H, W, B)
    Ho, Wo, pad, taps, use_pro = c["Ho"], c["Wo"], k // 2, k * k, c["use_pro"]
    geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=W, H_out=Ho, W_out=Wo, KH=k, KW=k, stride=s, pad=pad)
    wf = c["w"].permute(2, 3, 1, 0).reshape(-1).contiguous().to(dev)          # (tap, c, m)
    xd, dyd = cn(c["x"]).to(dev), cn(c["dy"]).to(dev)
    pro = (c["sc"].to(dev), c["sh"].to(dev)) if use_pro else None
    errs = {}
    if forward:
        out = torch.empty((cout, B * Ho * Wo), device=dev)
        r = ops.conv2d_gemm(xd, out, wf, cin * cout, cout, epi=L.SAR_EPI_STATS, pro=pro, pro_relu=use_pro, **geo)
        torch.cuda.synchronize()
        errs["y"] = rel_err(uncn(out.cpu(), B, Ho, Wo), c["y"])
        errs["ysq"] = rel_err(r[0].cpu().double().sum(1)[:, 1], c["ysq"])
    if wgrad:
        tmp = torch.empty(taps * cin * cout, device=dev)
        ops.conv2d_wgrad(xd, dyd, tmp, pro=pro, pro_relu=use_pro, **geo)
        torch.cuda.synchronize()
        errs["gw"] = rel_err(tmp.cpu().view(k, k, cin, cout).permute(3, 2, 0, 1), c["gw"])
    if dgrad:
        wb = c["w"].permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)      # (tap, m, c)
        dx = torch.empty((cin, B * H * W), device=dev)
        ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=c["add"].to(dev), B=B, Kc=cout, M=cin, H_src=Ho,
                        W_src=Wo, H_out=H, W_out=W, KH=k, KW=k, stride=s, pad=pad, transposed=True)
        torch.cuda.synchronize()
        errs["gh"] = rel_err(uncn(dx.cpu() - c["add"], B, H, W), c["gh"])
    _said(group, (cin, cout, k, s, H, W, B), **errs)
    assert all(e < TOL for e in errs.values()), errs


def _rect_masked_dgrad(group, cin, cout, s, H, W, B):
    """the data gradient with the MASK epilogue and both centred partial sums: (geo, dyd, wb, reference record)"""
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    c = RC.conv_ref(cin, cout, 3, s, H, W, B)
    Ho, Wo = c["Ho"], c["Wo"]
    wb = c["w"].permute(2, 3, 0, 1).reshape(-1).contiguous().to(dev)          # (tap, m, c)
    dyd = cn(c["dy"]).to(dev)
    geo = dict(B=B, Kc=cout, M=cin, H_src=Ho, W_src=Wo, H_out=H, W_out=W, KH=3, KW=3, stride=s, pad=1, transposed=True)
    dx = torch.empty((cin, B * H * W), device=dev)
    r = ops.conv2d_gemm(dyd, dx, wb, cout * cin, cin, epi=L.SAR_EPI_MASK, aux=c["aux"].to(dev),
                        aux_affine=(c["sc2"].to(dev), c["sh2"].to(dev)), aux_mean=c["mu"].to(dev), **geo)
    torch.cuda.synchronize()
    part = r[0].cpu().double().sum(1)
    errs = _said(group, (cin, cout, s, H, W, B), dz=rel_err(dx.cpu(), c["dz"]), dz_sum=rel_err(part[:, 0], c["dz_sum"]),
                 dz_cen=rel_err(part[:, 1], c["dz_cen"]))
    assert errs["dz"] < TOL and errs["dz_sum"] < 1e-4 and errs["dz_cen"] < 1e-4, errs
    return geo, dyd, wb, c


@pytest.mark.parametrize("cin,cout,H,W", RC.A_PARITY + RC.A_MASKED)
def test_rect_stride2_data_gradient(cin, cout, H, W):
    """A. 3x3 / stride 2 / pad 1 data gradient onto an H x W image: both sides even -> the four parity-class launches (MASK partials
    spread over them, the compact even-pixel aux indexed Ho x Wo); H or W odd -> the masked kernel, which has no compact aux: the
    call raises and writes nothing."""
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    B = RC.A_BATCH
    geo, dyd, wb, c = _rect_masked_dgrad("A", cin, cout, 2, H, W, B)
    if (cin, cout, H, W) in RC.A_PARITY:
        assert RC.dgrad_s2_route(H, W) == "parity"
        dx2 = torch.empty((cin, B * H * W), device=dev)
        ops.conv2d_gemm(dyd, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=c["small"].to(dev), aux_even_pixels=True, **geo)
        torch.cuda.synchronize()
        errs = _said("A", (cin, cout, 2, H, W, B), gh_even=rel_err(uncn(dx2.cpu(), B, H, W), c["gh_even"]))
        assert errs["gh_even"] < TOL
    else:
        assert RC.dgrad_s2_route(H, W) == "masked"
        dx2 = torch.full((cin, B * H * W), -7.25, device=dev)
        with pytest.raises(L.SarError):
            ops.conv2d_gemm(dyd, dx2, wb, cout * cin, cin, epi=L.SAR_EPI_ADD, aux=c["small"].to(dev), aux_even_pixels=True, **geo)
        torch.cuda.synchronize()
        assert bool((dx2 == -7.25).all())


@pytest.mark.parametrize("cin,cout,H,W", RC.B_CASES)
def test_rect_1x1_stride2(cin, cout, H, W):
    """B. the down-sampling convolution: forward with STATS, data gradient, weight gradient"""
    _rect_conv("B", cin, cout, 1, 2, H, W, 2)


@pytest.mark.parametrize("cout,H,W", RC.C_CASES)
def test_rect_stem_forward_and_weight_gradient(cout, H, W):
    """C. stem 7x7 / stride 2 / pad 3 on one input channel"""
    _rect_conv("C", 1, cout, 7, 2, H, W, 2, dgrad=False)


def _stem_dgrad_operands(case, dev):
    c = RC.stem_dgrad_ref(*case)
    return c, cn(c["dout"]).to(dev), c["w"].permute(2, 3, 1, 0).reshape(-1).contiguous().to(dev)      # [k*k][1][M]


@pytest.mark.parametrize("case", RC.D_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_stem_data_gradient_called_directly(case):
    """D. sar_conv2d_stem_dgrad_f32 at any (k, stride, pad) against the float64 autograd of F.conv2d with one input channel"""
    from sar_amd import ops
    dev = torch.device("cuda:0")
    B, M, H, W, k, s, p = case
    c, dout, wp = _stem_dgrad_operands(case, dev)
    dx = torch.empty((B, 1, H, W), device=dev)
    ops.conv2d_stem_dgrad(dout, wp, dx, B=B, H=H, W=W, H_out=c["Ho"], W_out=c["Wo"], M=M, KH=k, KW=k, stride=s, pad=p)
    torch.cuda.synchronize()
    errs = _said("D", case, dx=rel_err(dx.cpu(), c["dx"]))
    assert errs["dx"] < TOL


def test_stem_data_gradient_padded_dout_and_guarded_dx():
    """D. dout a view with ld_dout > B Ho Wo inside NaN, dx inside a guarded flat range: the result is the tight launch's, bit for
    bit, finite, and nothing around dx is written"""
    from sar_amd import ops
    from util import NAN, SENTINEL, assert_flat_guards_untouched, guarded, guarded_flat
    dev = torch.device("cuda:0")
    case = (2, 64, 17, 11, 5, 2, 2)
    B, M, H, W, k, s, p = case
    c, dout, wp = _stem_dgrad_operands(case, dev)
    geo = dict(B=B, H=H, W=W, H_out=c["Ho"], W_out=c["Wo"], M=M, KH=k, KW=k, stride=s, pad=p)
    tight = torch.empty((B, 1, H, W), device=dev)
    ops.conv2d_stem_dgrad(dout, wp, tight, **geo)
    for pad in (4, 7):
        view, _ = guarded(dout, pad, NAN, dev)
        dx, whole = guarded_flat(B * H * W, SENTINEL, dev)
        assert view.stride(0) == B * c["Ho"] * c["Wo"] + pad
        ops.conv2d_stem_dgrad(view, wp, dx, **geo)
        torch.cuda.synchronize()
        assert_flat_guards_untouched(whole, B * H * W, SENTINEL, what="dx (pad %d)" % pad)
        assert bool(torch.isfinite(dx).all()) and torch.equal(dx.view(B, 1, H, W), tight)
        assert rel_err(dx.cpu().view(B, 1, H, W), c["dx"]) < TOL


def test_stem_data_gradient_rejects_bad_arguments():
    """D. ld_dout below B Ho Wo, a weight tile above 64 KiB of LDS, a null pointer: the error code, and dx still holds its fill"""
    from sar_amd import ops, _lib as L
    dev = torch.device("cuda:0")
    case = (3, 5, 9, 14, 3, 1, 1)
    B, M, H, W, k, s, p = case
    c, dout, wp = _stem_dgrad_operands(case, dev)
    n = B * c["Ho"] * c["Wo"]
    geo = dict(B=B, H=H, W=W, H_out=c["Ho"], W_out=c["Wo"], M=M, KH=k, KW=k, stride=s, pad=p)
    dx = torch.full((B, 1, H, W), -7.25, device=dev)
    with pytest.raises(L.SarError):                                   # rows of n - 1 columns under a live width of n
        ops.conv2d_stem_dgrad(dout[:, :n - 1].contiguous(), wp, dx, **geo)
    big = 400                                                         # 7 * 7 * 400 * 4 = 78 400 bytes > 64 KiB
    with pytest.raises(L.SarError):
        ops.conv2d_stem_dgrad(torch.zeros((big, n), device=dev), torch.zeros(49 * big, device=dev), dx,
                              **dict(geo, M=big, KH=7, KW=7, stride=1, pad=3))
    lib = L.load()
    args = (B, H, W, c["Ho"], c["Wo"], M, k, k, s, p)
    for d_, w_, x_ in ((None, L.ptr(wp), L.ptr(dx)), (L.ptr(dout), None, L.ptr(dx)), (L.ptr(dout), L.ptr(wp), None)):
        assert lib.sar_conv2d_stem_dgrad_f32(d_, dout.stride(0), w_, *args, x_, L.stream_ptr()) == L.SAR_E_ARG
    torch.cuda.synchronize()
    assert bool((dx == -7.25).all())


@pytest.mark.parametrize("B,C,H,W", RC.E_CASES)
def test_rect_stem_tail_maxpool_forward_backward(B, C, H, W):
    """E. bn + relu + max-pool and its backward on an H x W image; (18, 131) and (17, 260) give the backward a 2 x 2 and a 2 x 3 grid of
    16 x 128 tiles: the halo across column 128, tr / tiles_w and tr % tiles_w, partials ordered over a 2-D grid"""
    from sar_amd import ops
    dev = torch.device("cuda:0")
    c = RC.maxpool_ref(B, C, H, W)
    Ho, Wo = c["Ho"], c["Wo"]
    xd = cn(c["x"]).to(dev)
    yd = torch.empty((C, B * Ho * Wo), device=dev)
    scd, shd = c["sc"].to(dev), c["sh"].to(dev)
    ops.bn_relu_maxpool_fwd(xd, scd, shd, yd, B, H, W)
    dz = torch.empty_like(xd)
    part, nparts = ops.bn_relu_maxpool_bwd(xd, scd, shd, c["mean"].float().to(dev), cn(c["dy"]).to(dev), dz, B, H, W)
    torch.cuda.synchronize()
    th, tw = RC.mpb_tiles(H, W)
    assert nparts == B * th * tw
    ps = part.cpu().double().sum(1)
    errs = _said("E", (B, C, H, W), y=rel_err(uncn(yd.cpu(), B, Ho, Wo), c["y"]), gz=rel_err(uncn(dz.cpu(), B, H, W), c["gz"]),
                 gz_sum=rel_err(ps[:, 0], c["gz_sum"]), gz_cen=rel_err(ps[:, 1], c["gz_cen"]))
    assert errs["y"] < TOL and errs["gz"] < TOL and errs["gz_sum"] < 1e-4 and errs["gz_cen"] < 1e-4, errs


@pytest.mark.parametrize("cin,cout,s,H,W", RC.F_ALL)
def test_rect_weight_gradient_fixed_geometry_variants(cin, cout, s, H, W):
    """F. 3x3 weight gradient: W_out in {64, 32, 16, 8} with H_out no multiple of the row tile puts a ragged last tile through the
    compile-time loop of v0..v6 (tests/test_conv2d_rect_cases.py names the variant per case); the H / W twins take the generic loop"""
    _rect_conv("F", cin, cout, 3, s, H, W, 2, forward=False, dgrad=False)


@pytest.mark.parametrize("cin,cout,H,W,B", RC.G_CASES)
def test_rect_small_maps_share_a_tile(cin, cout, H, W, B):
    """G. 3x3 / stride 1 on 3 x 5, 2 x 3 and 4 x 4 maps: several whole images in one tile (NI > 1): forward with STATS and the
    masked data gradient"""
    assert RC.gemm_images_per_tile(B, H, W, False)[0] > 1
    _rect_conv("G", cin, cout, 3, 1, H, W, B, wgrad=False, dgrad=False)
    _rect_masked_dgrad("G", cin, cout, 1, H, W, B)
