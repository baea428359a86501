"""Rectangular and odd-sized cases for the 2-D convolution path (csrc/conv2d*.hip, the ResNet-18 engine of sar_amd/resnet.py): the case
tables, their float64 references and a Python restatement of the host-side tile choices.  A helper, not a test:
tests/test_conv2d_rect_cases.py pins the tables on the CPU, tests/test_gpu_conv2d_kernels.py and the two guard-band suites run them.

References are torch.nn.functional.conv2d / max_pool2d with autograd, float64 by default; dtype=torch.float32 evaluates the SAME inputs
(generated in float32) in float32 (the conditioning band), control="hw" re-evaluates the same flat buffers read as (W, H) images and
control="batch" with images 0 and 1 exchanged (the sensitivity controls: a case whose reference survives them is not in a table).

Groups (the issue's letters):
  A  3x3 / stride 2 / pad 1 data gradient: both sides even -> four parity-class launches; else the masked kernel
  B  1x1 / stride 2 (the down-sampling branch)
  C  stem 7x7 / stride 2 / pad 3, one input channel: forward and weight gradient
  D  stem data gradient (sar_conv2d_stem_dgrad_f32), any (k, stride, pad)
  E  bn + relu + max-pool(3, 2, 1) forward and backward; the backward tiles the image 16 x 128
  F  3x3 weight gradient: the fixed-geometry variants v0..v6 with a ragged last row tile, and their H/W twins (generic loop)
  G  3x3 / stride 1 on maps small enough that several whole images share one tile (NI > 1)"""
import functools

import torch
import torch.nn.functional as F

F64 = torch.float64

# ---------------------------------------------------------------------------------------------------- the tables
# A: (cin, cout, H, W), B = 3
A_PARITY = [(16, 32, 12, 20), (8, 16, 8, 36), (16, 32, 20, 12)]
A_MASKED = [(8, 16, 12, 15), (8, 16, 15, 12), (8, 16, 13, 18)]
A_BATCH = 3
# B: (cin, cout, H, W), B = 2
B_CASES = [(16, 32, 12, 20), (8, 16, 13, 18)]
# C: (cout, H, W), B = 2
C_CASES = [(8, 20, 36), (40, 25, 35), (8, 36, 20)]
# D: (B, M, H, W, k, s, p): the geometries of C, then every (k, s, p) at two shapes whose B H W is no multiple of 256
D_KSP = [(3, 1, 1), (5, 2, 2), (1, 2, 0), (7, 2, 3)]
D_CASES = [(2, cout, H, W, 7, 2, 3) for cout, H, W in C_CASES] + \
          [(B, M, H, W, k, s, p) for (B, M, H, W) in [(3, 5, 9, 14), (2, 64, 17, 11)] for (k, s, p) in D_KSP]
# E: (B, C, H, W)
E_CASES = [(2, 8, 12, 20), (3, 5, 25, 35), (1, 4, 18, 131), (2, 3, 17, 260)]
# F: (cin, cout, stride, H, W) -> intended variant; B = 2.  The twin of a case is the same with H and W exchanged.
F_CASES = [((8, 8, 1, 5, 64), 0), ((8, 8, 1, 6, 32), 1), ((8, 16, 2, 10, 64), 2), ((24, 40, 1, 11, 16), 3), ((8, 16, 2, 10, 32), 4),
           ((8, 8, 1, 7, 8), 5), ((8, 16, 2, 14, 16), 6)]
F_TWINS = [(cin, cout, s, W, H) for (cin, cout, s, H, W), _ in F_CASES]
F_ALL = [c for c, _ in F_CASES] + F_TWINS
# G: (cin, cout, H, W, B)
G_CASES = [(32, 32, 3, 5, 3), (32, 32, 3, 5, 7), (64, 64, 2, 3, 5), (32, 32, 4, 4, 7)]

TOL, TOL_SUM = 2e-5, 1e-4      # the project's bars: tensors, reduced partial sums


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------------------------------- the controls
def _hw(t, on):
    """the flat buffer of a (B, C, H, W) tensor read as (B, C, W, H) -- and back"""
    return t.reshape(t.shape[0], t.shape[1], t.shape[3], t.shape[2]) if on else t


def _batch(t, on):
    """images 0 and 1 exchanged"""
    if not on:
        return t
    idx = list(range(t.shape[0]))
    idx[0], idx[1] = 1, 0
    return t[idx]


def cn(x):     # (B,C,H,W) -> [C][B*H*W]
    B, C, H, W = x.shape
    return x.permute(1, 0, 2, 3).reshape(C, B * H * W).contiguous()


# ---------------------------------------------------------------------------------------------------- the references
@functools.lru_cache(maxsize=None)
def conv_ref(cin, cout, k, s, H, W, B, dtype=F64, control=None):
    """conv2d(k x k, stride s, pad k // 2) behind a folded BatchNorm + ReLU where cin > 1 (tests/test_gpu_conv2d_kernels.py:
    test_conv2d_forward_dgrad_wgrad), its gradients, and the operands of the data gradient's epilogues
    (test_stride2_data_gradient_parity_classes): aux / sc2 / sh2 / mu the MASK operands, small the compact even-pixel aux, add the ADD
    operand.  Every input is drawn in float32, so every dtype evaluates the same numbers."""
    hw, bt = control == "hw", control == "batch"
    pad, taps = k // 2, k * k
    Ho, Wo = out_size(H, k, s, pad), out_size(W, k, s, pad)
    g = torch.Generator().manual_seed(1000 * H + 10 * W + cin * 7 + cout + k + s)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * taps) ** 0.5
    sc, sh = 1 + 0.2 * torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g)
    dy = torch.randn(B, cout, Ho, Wo, generator=g)
    aux, add = torch.randn(cin, B * H * W, generator=g), torch.randn(cin, B * H * W, generator=g)
    sc2, sh2, mu = 1 + 0.2 * torch.randn(cin, generator=g), 0.3 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    small = torch.randn(cin, B * Ho * Wo, generator=g)
    use_pro = cin > 1
    xe = _hw(_batch(x, bt), hw).to(dtype)
    hin = torch.relu(xe * sc.to(dtype).view(1, -1, 1, 1) + sh.to(dtype).view(1, -1, 1, 1)) if use_pro else xe
    hin = hin.detach().requires_grad_(True)
    wq = w.to(dtype).requires_grad_(True)
    y = F.conv2d(hin, wq, None, stride=s, padding=pad)
    gh, gw = torch.autograd.grad(y, (hin, wq), _hw(_batch(dy, bt), hw).to(dtype))
    y, gh = _hw(y.detach(), hw), _hw(gh, hw)
    mask = (aux.to(dtype) * sc2.to(dtype)[:, None] + sh2.to(dtype)[:, None]) > 0
    dz = cn(gh) * mask
    full = torch.zeros(B, cin, H, W, dtype=dtype)
    if H == 2 * Ho and W == 2 * Wo:
        full[:, :, ::2, ::2] = small.to(dtype).reshape(cin, B, Ho, Wo).permute(1, 0, 2, 3)
    return dict(x=x, w=w, sc=sc, sh=sh, use_pro=use_pro, dy=dy, aux=aux, add=add, sc2=sc2, sh2=sh2, mu=mu, small=small, Ho=Ho, Wo=Wo,
                y=y, ysq=(y * y).sum(dim=(0, 2, 3)), gh=gh, gw=gw, dz=dz, dz_sum=dz.sum(1),
                dz_cen=(dz * (aux.to(dtype) - mu.to(dtype)[:, None])).sum(1), gh_even=gh + full)


@functools.lru_cache(maxsize=None)
def stem_dgrad_ref(B, M, H, W, k, s, p, dtype=F64, control=None):
    """image gradient of a one-input-channel convolution: autograd of F.conv2d"""
    hw = control == "hw"
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    g = torch.Generator().manual_seed(100 * H + W + 7 * M + k + s + p)
    dout = torch.randn(B, M, Ho, Wo, generator=g)
    w = torch.randn(M, 1, k, k, generator=g) / (k * k) ** 0.5
    x = torch.zeros(B, 1, *((W, H) if hw else (H, W)), dtype=dtype, requires_grad=True)
    y = F.conv2d(x, w.to(dtype), None, stride=s, padding=p)
    (dx,) = torch.autograd.grad(y, x, _hw(dout, hw).to(dtype))
    return dict(dout=dout, w=w, dx=_hw(dx, hw), Ho=Ho, Wo=Wo)


@functools.lru_cache(maxsize=None)
def maxpool_ref(B, C, H, W, dtype=F64, control=None):
    """max_pool2d(relu(x * sc + sh), 3, 2, 1) and its gradient w.r.t. the BatchNorm output (test_stem_tail_maxpool_forward_backward)"""
    hw = control == "hw"
    Ho, Wo = out_size(H, 3, 2, 1), out_size(W, 3, 2, 1)
    g = torch.Generator().manual_seed(3 + 100 * H + W)
    x = torch.randn(B, C, H, W, generator=g)
    sc, sh = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B, C, Ho, Wo, generator=g)
    xe = _hw(x, hw).to(dtype).requires_grad_(True)
    y = F.max_pool2d(torch.relu(xe * sc.to(dtype).view(1, -1, 1, 1) + sh.to(dtype).view(1, -1, 1, 1)), 3, 2, 1)
    (gx,) = torch.autograd.grad(y, xe, _hw(dy, hw).to(dtype))
    gz = _hw(gx, hw) / sc.to(dtype).view(1, -1, 1, 1)
    xd = x.to(dtype)
    mean = xd.mean(dim=(0, 2, 3))
    return dict(x=x, sc=sc, sh=sh, dy=dy, Ho=Ho, Wo=Wo, y=_hw(y.detach(), hw), gz=gz, mean=mean, gz_sum=gz.sum(dim=(0, 2, 3)),
                gz_cen=(gz * (xd - mean.view(1, -1, 1, 1))).sum(dim=(0, 2, 3)))


# ---------------------------------------------------------------------------------------------------- the host's tile choices, restated
# csrc/conv2d.hip: SAR_C2D_WG_VARIANTS, (W_out, stride, RP) of v0..v6
WG_VARIANTS = [(64, 1, 1), (32, 1, 2), (32, 2, 1), (16, 1, 4), (16, 2, 2), (8, 1, 4), (8, 2, 4)]
MPB_TH, MPB_TW = 16, 128


def wgrad_tile(H_out, W_out, W_src, stride, pad, KH, KW, stem=False, WF=2, WC=1, WT=2, TPW=5, DJ=4, SJMAX=12):
    """launch_wgrad's row tile: dict(th, RP, TPI) or None (does not fit).  The defaults are the 3x3 instantiation."""
    taps, BF, CT = KH * KW, 32 * WF, 1 if stem else 32 * WC
    th = (32 * DJ // W_out) & ~1
    if th < 2:
        return None
    th = min(th, (H_out + 1) & ~1)
    while True:
        NPOS, NR, Wq = th * W_out, (th - 1) * stride + KH, W_src + 2 * pad
        RW = NR * Wq
        SP = (RW + (0 if stem else (WT * TPW - taps) * (Wq + KW))) | 1
        lds = 4 * (BF * (NPOS | 1) + CT * SP)
        if (lds <= 78 * 1024 and RW <= (256 if stem else 32) * SJMAX and NPOS <= 32 * DJ) or th == 2:
            break
        th -= 2
    if NPOS > 32 * DJ or RW > (256 if stem else 32) * SJMAX or lds > 150 * 1024:
        return None
    return dict(th=th, RP=th // 2, TPI=-(-H_out // th))


def wgrad3x3_route(H, W, stride):
    """sar_c2d_wgrad for 3x3 / pad 1 on an H x W source: ("v<i>" | "generic", tile)"""
    H_out, W_out = out_size(H, 3, stride, 1), out_size(W, 3, stride, 1)
    t = wgrad_tile(H_out, W_out, W, stride, 1, 3, 3)
    for i, (WO, SD, RPC) in enumerate(WG_VARIANTS):
        if W_out == WO and stride == SD:      # the dispatch key; the variant itself falls back unless its tile shape holds
            if t is not None and t["RP"] == RPC and W + 2 == WO * SD + 2:
                return "v%d" % i, t
            break
    return "generic", t


def dgrad_s2_route(H, W):
    """sar_c2d_gemm_transposed for 3x3 / stride 2 / pad 1 onto an H x W image: the parity classes need H = 2 Ho and W = 2 Wo"""
    return "parity" if H == 2 * out_size(H, 3, 2, 1) and W == 2 * out_size(W, 3, 2, 1) else "masked"


def mpb_tiles(H, W):
    """bn_relu_maxpool_bwd: (tiles_h, tiles_w)"""
    return -(-H // MPB_TH), -(-W // MPB_TW)


def gemm_images_per_tile(B, H, W, transposed, tile_n=256, rwmax=640):
    """gemm_geometry for 3x3 / stride 1 / pad 1 at M <= 64 (256-column tiles): (NI, ntiles)"""
    th = min(tile_n // W, H)
    while True:
        NR, Wq = (th + 2, W + 2) if not transposed else (th + 3, W + 2)
        if NR * Wq <= rwmax or th == 1:
            break
        th -= 1
    NI, TPI = 1, -(-H // th)
    if th == H and 2 * H * W <= tile_n:
        NI = min(tile_n // (H * W), B)
        while NI > 1 and NI * NR * Wq > rwmax:
            NI -= 1
    return NI, (-(-B // NI) if NI > 1 else B * TPI)


# ---------------------------------------------------------------------------------------------------- the route table
# what each case is in the table FOR.  `split`: ops.conv2d_split_applicable of the launch named (the kernel the f32_split arithmetic runs).
ROUTES = (
    [dict(group="A", case=c, dgrad="parity", split=True) for c in A_PARITY] +
    [dict(group="A", case=c, dgrad="masked", split=False) for c in A_MASKED] +
    [dict(group="E", case=(2, 8, 12, 20), tiles=(1, 1)), dict(group="E", case=(3, 5, 25, 35), tiles=(2, 1)),
     dict(group="E", case=(1, 4, 18, 131), tiles=(2, 2)), dict(group="E", case=(2, 3, 17, 260), tiles=(2, 3))] +
    [dict(group="F", case=c, wgrad="v%d" % v, ragged=True) for c, v in F_CASES] +
    [dict(group="F", case=c, wgrad="generic") for c in F_TWINS] +
    [dict(group="G", case=(32, 32, 3, 5, 3), NI=3, ntiles=1, split=False), dict(group="G", case=(32, 32, 3, 5, 7), NI=7, ntiles=1, split=False),
     dict(group="G", case=(64, 64, 2, 3, 5), NI=5, ntiles=1, split=False), dict(group="G", case=(32, 32, 4, 4, 7), NI=7, ntiles=1, split=False)]
)
