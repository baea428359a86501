"""bs = 64 (B = N*M = 128 sequences, T = 300) for the bf16 engine's CN8 kernels (BASELINE configs[2]; engine mfma="bf16").

tests/test_gpu_batch64.py's method applied to sar_amd/ops8.py, with float64 anchors because the 2-sequence slice launches must
themselves be right.  Every launch is set up as sar_amd/stgcn8.py sets it up: the engine's packed bf16 weight images, its gather
tables (SAR_GRAPH_FEW_DENSE -> the read-gather graph kernels), its epilogues (STATS, MASK with aux_affine, ADD / ADD_GATE with
aux2 / aux_mask / aux_mean), the block tail's ReLU mask and the engine's persistent SlabBatch.  Environment switches stay at
their defaults.  For the six block geometries of test_gpu_batch64.LAYERS (blocks l0, l1, l4, l5, l7, l8, each with its own
residual kind):

  * outputs and ReLU masks of the B = 128 launch equal BIT FOR BIT the launches on 2-sequence slices 0, 1, 31, 62, 63 (a
    workgroup tile is whole frames of one sequence; BatchNorm enters as per-channel vectors);
  * partial sums and weight gradients of the B = 128 launch equal the float64 sum of all 64 slice launches to <= 2e-6 (a
    bf16 x bf16 product is exact in fp32, so both sides differ only by fp32 summation order over the reduction lengths of the
    fp32 engine's suite);
  * slice 0 of every launch equals its float64 definition (tests/test_gpu_cn8.py's: stored outputs within one bf16 rounding,
    weight gradients 1e-5, partial sums 1e-4), and the BatchNorm-backward sums of the B = 128 launches equal float64 sums of
    the stored bf16 tensors computed on the device;
  * eval-mode logits of the bf16 engine at bs = 64 equal 2-clip forwards bit for bit.

Every B = 128 output is NaN-filled before its launch, and so is the memory the wrappers' partial-sum buffers are allocated
from (the caching allocator hands a block just released to the next request of the same size): an unwritten tile or partial
cannot pass.  The weight gradients go through the engine's SlabBatch with the slab NaN-filled; at l0 / l1 the 9-tap temporal
weight gradient has splits without tiles (ops8.conv_wgrad: nsplit = 512 / blocks > ntiles / tps), which must still write
their zero rows.  The slice launches take NaN-filled slabs of their own (at B = 2, l7 / l8 have empty splits too).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import stgcn as O
from util import assert_bf16_close, bf as _bf, from_cn, graph_ref, rel_err

pytestmark = pytest.mark.gpu
V, B = 25, 128
KS, KT = 3, 9
# (cin, f, stride, T, block): the six distinct geometries of test_gpu_batch64.LAYERS and the block of the default ST-GCN they are
LAYERS = [(3, 64, 1, 300, 0), (64, 64, 1, 300, 1), (64, 128, 2, 300, 4), (128, 128, 1, 150, 5), (128, 256, 2, 150, 7),
          (256, 256, 1, 75, 8)]
SLICES = [0, 1, 31, 62, 63]           # 2-sequence slices compared bit for bit (first, second, middle, last two)
RED_TOL = 2e-6                        # B = 128 reduction vs the float64 sum of the slice launches
# B = 128 BatchNorm-backward sums vs float64 sums of the stored bf16 tensors: fp32 summation order only, per channel relative to
# its sum of |terms| (measured <= 3e-8 for the reduce pass and the ADD_GATE epilogue).  The MASK epilogue sums its unrounded
# fp32 accumulators instead: see _anchor.
SUM_TOL = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def eng(dev):
    """the bf16 engine with randomised affine / BatchNorm state (oracle.stgcn.randomize_affine) and its BatchNorm vectors (scale,
    shift from the moving statistics; mean, rstd; backward constants k1..k3) set as a step would leave them"""
    from sar_amd.stgcn import STGCN, BN_EPS
    e = STGCN(num_classes=60, device=dev, seed=11, mfma="bf16")
    for cin, f, s, T, blk in LAYERS:
        assert e.blocks[blk][:2] == (f, s) and (blk == 0 or e.blocks[blk - 1][0] == cin)
    st = e.state_dict()
    st.pop("A")
    e.load_params(O.randomize_affine(st, seed=12))
    e.packed.refresh(e.flat)
    g = torch.Generator(device=dev).manual_seed(13)
    for name, bn in e.bn.items():
        e._bn_eval(name)
        bn.mean.copy_(bn.moving_mean)
        bn.rstd.copy_(torch.rsqrt(bn.moving_var + BN_EPS))
        for k in (bn.k1, bn.k2, bn.k3):
            k.copy_(0.5 * torch.randn(k.shape, generator=g, device=dev))
    torch.cuda.synchronize()
    return e


def _rand8(C, n, dev, seed):
    from sar_amd import ops8
    g = torch.Generator(device=dev).manual_seed(seed)
    return ops8.from_cn(torch.randn((C, n), generator=g, device=dev))


def _cols(t, T, i, n=2):
    """contiguous copy of the columns of sequences [n*i, n*i + n) (CN8 tensor or ReLU mask)"""
    w = T * V
    return t[:, n * i * w:(n * i + n) * w].contiguous()


def _same_pad(T, k, s):
    out = -(-T // s)
    total = max((out - 1) * s + k - T, 0)
    return out, total // 2


def _cn(x8, C):
    """CN8 -> float64 CN matrix on the device"""
    from sar_amd import ops8
    return ops8.to_cn(x8, C).double()


def _back(x8, C, nb, T):
    from sar_amd import ops8
    return from_cn(ops8.to_cn(x8, C).cpu(), nb, T, V).double()


def _mask_bits(m, C):
    """(planes, n) gate / ReLU-mask bytes -> (C, n) bool: bit j of byte (g, col) = channel 8 g + j"""
    bits = (m.to(torch.int32).unsqueeze(1) >> torch.arange(8, device=m.device, dtype=torch.int32).view(1, 8, 1)) & 1
    return bits.reshape(-1, m.shape[1])[:C].bool()


def _poisoned(run, outs, dev):
    """run() at B = 128 behind NaN-filled outputs (0xA5 mask bytes) and NaN-filled partial-sum memory.  A first launch learns the
    shape of the partials the wrapper allocates; the block of that size is then filled with NaN and released, and the caching
    allocator hands that same block to the second launch's torch.empty (same pool state, same request).  The two launches must
    agree bit for bit."""
    first = run()
    ref = [t.clone() for t in outs]
    shape = None if first is None else tuple(first[0].shape)
    first_p = None if first is None else first[0].clone()
    del first
    for t in outs:
        t.fill_(float("nan") if t.is_floating_point() else 0xA5)
    addr = None
    if shape is not None:
        trap = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        addr = trap.data_ptr()
        del trap
    r = run()
    if shape is not None:
        assert r[0].data_ptr() == addr, "the partial-sum buffer did not come from the NaN-filled block"
        assert torch.equal(r[0], first_p), "partial sums differ between two identical B = 128 launches"
    for a, b in zip(outs, ref):
        assert torch.equal(a, b), "outputs differ between two identical B = 128 launches"
    return r


def _psum(r):
    return r[0].double().sum(dim=1)          # [M][nsum]


def _full_vs_slices(what, full, sums, stats=False):
    """BatchNorm statistics (sum, sum of squares): the sum is cancelled (mean ~ 0), so both are measured against the
    sum-of-squares scale; backward sums (centred): against their largest entry, as in the fp32 suite"""
    scale = (sums[:, 1] if stats else sums).abs().max().item()
    err = (full - sums).abs().max().item() / scale
    print("%s: B=128 partial sums vs float64 sum of the 64 slice launches: %.2e of scale" % (what, err))
    assert err < RED_TOL, what


def _anchor(what, part, terms, ulps=None):
    """summed partials [C][j] of a B = 128 launch vs float64 sums of terms[j] ((C, n) float64 on the device), per channel within
    SUM_TOL of its sum of |terms|.  ulps[j] ((C, n)): where the kernel summed its unrounded fp32 accumulators and the terms hold
    the stored bf16 values, the size of one bf16 ulp of each term: the two sums then also differ by n independent roundings to
    nearest, each uniform within half an ulp (variance ulp^2 / 12), and 6 standard deviations of that sum are allowed on top.
    (A fixed fraction of the sum of |terms| would not do: that sum grows like n, the rounding noise like sqrt(n) -- measured
    4.7e-6 .. 1.7e-5 of it across the layers.)"""
    for j, t in enumerate(terms):
        absum = t.abs().sum(dim=1)
        diff = (part[:, j] - t.sum(dim=1)).abs()
        tol = SUM_TOL * absum
        msg = "%.2e of sum |terms|" % (diff / absum).max().item()
        if ulps is not None:
            sigma = (ulps[j] ** 2 / 12).sum(dim=1).sqrt()
            tol = tol + 6 * sigma
            msg += ", %.2f sigma of the bf16 rounding" % (diff / sigma).max().item()
        print("%s: B=128 sum %d vs float64 of the stored tensors: %s" % (what, j, msg))
        assert (diff <= tol).all(), (what, j)


def _ulp(x):
    """one bfloat16 ulp of every (bf16-valued) element, 0 at 0"""
    e = torch.frexp(x).exponent
    return torch.ldexp(torch.ones_like(x), e - 8) * (x != 0)


def _slice_partials_close(what, part, ref_sum, ref_abs=None):
    """slice-0 partial sums vs float64: rel_err 1e-4 (a cancelled first sum: 1e-4 of its sum of |terms|)"""
    part = part.cpu()
    err = rel_err(part, ref_sum) if ref_abs is None else (part - ref_sum).abs().max().item() / ref_abs.max().item()
    print("%s: slice 0 partial sums vs float64 definition: %.2e" % (what, err))
    assert err < 1e-4, what


# ----------------------------------------------------------------------------------------------------------------- 1. forward

@pytest.mark.parametrize("cin,f,s,T,blk", LAYERS)
def test_forward_at_bs64_equals_slices_and_float64(dev, eng, cin, f, s, T, blk):
    from sar_amd import ops8, _lib as L
    pre, kind = "l%d." % blk, eng.kinds[blk]
    To, pad = _same_pad(T, KT, s)
    n_in, n_out = B * T * V, B * To * V
    img = eng.packed.image
    bn1, bn2, rbn = eng.bn[pre + "bn1"], eng.bn[pre + "bn2"], eng.bn.get(pre + "res_bn")
    res_kind = {"none": 0, "identity": 1, "conv": 2}[kind]
    print("l%d (%s): cin %d f %d stride %d T %d -> %d" % (blk, kind, cin, f, s, T, To))
    X = _rand8(cin, n_in, dev, 100 + blk)

    def graph(x, nb, out):
        return ops8.conv_gemm(L.SAR_CONV_GRAPH, x, out, img(pre + "gcn.f"), B=nb, V=V, T_src=T, T_out=T, Kc=cin, M=f, taps=KS,
                              bias=eng.p[pre + "gcn.bias"], tables=eng.tab_fwd, epi=L.SAR_EPI_STATS)

    def temporal(g_, nb, out):
        return ops8.conv_gemm(L.SAR_CONV_TEMPORAL, g_, out, img(pre + "tcn.f"), B=nb, V=V, T_src=T, T_out=To, Kc=f, M=f, taps=KT,
                              stride=s, pad=pad, bias=eng.p[pre + "tcn.bias"], pro=(bn1.scale, bn1.shift), pro_relu=True,
                              epi=L.SAR_EPI_STATS)

    def residual(x, nb, out):
        return ops8.conv_gemm(L.SAR_CONV_TEMPORAL, x, out, img(pre + "res.f"), B=nb, V=V, T_src=T, T_out=To, Kc=cin, M=f, taps=1,
                              stride=s, pad=0, bias=eng.p[pre + "res.bias"], epi=L.SAR_EPI_STATS)

    def tail(u, x, r, y, m):
        ops8.bn_add_relu_fwd(u, bn2.scale, bn2.shift, res_kind, x if kind == "identity" else r, rbn.scale if rbn else None,
                             rbn.shift if rbn else None, y, f, mask=m)

    g = ops8.empty(f, n_in, dev)
    rg = _poisoned(lambda: graph(X, B, g), [g], dev)
    u = ops8.empty(f, n_out, dev)
    ru = _poisoned(lambda: temporal(g, B, u), [u], dev)
    r = rr = None
    if kind == "conv":
        r = ops8.empty(f, n_out, dev)
        rr = _poisoned(lambda: residual(X, B, r), [r], dev)
    y, ym = ops8.empty(f, n_out, dev), ops8.relu_mask(f, n_out, dev)
    _poisoned(lambda: tail(u, X, r, y, ym), [y, ym], dev)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    sums = {k: torch.zeros((f, 2), dtype=torch.float64, device=dev) for k in ("g", "u", "r")}
    s0 = None
    for i in range(B // 2):
        xs = _cols(X, T, i)
        gs, us = ops8.empty(f, 2 * T * V, dev), ops8.empty(f, 2 * To * V, dev)
        r1 = graph(xs, 2, gs)
        r2 = temporal(_cols(g, T, i), 2, us)
        sums["g"] += _psum(r1)
        sums["u"] += _psum(r2)
        rs = None
        if kind == "conv":
            rs = ops8.empty(f, 2 * To * V, dev)
            r3 = residual(xs, 2, rs)
            sums["r"] += _psum(r3)
        if i in SLICES:
            ys, ms = ops8.empty(f, 2 * To * V, dev), ops8.relu_mask(f, 2 * To * V, dev)
            tail(us, xs, rs, ys, ms)
            assert torch.equal(gs, _cols(g, T, i)), "graph conv, slice %d" % i
            assert torch.equal(us, _cols(u, To, i)), "temporal conv, slice %d" % i
            assert rs is None or torch.equal(rs, _cols(r, To, i)), "residual conv, slice %d" % i
            assert torch.equal(ys, _cols(y, To, i)), "block tail, slice %d" % i
            assert torch.equal(ms, _cols(ym, To, i)), "ReLU mask, slice %d" % i
        if i == 0:
            s0 = dict(x=xs, g_in=_cols(g, T, 0), gs=gs, us=us, rs=rs, r1=r1, r2=r2, r3=r3 if rs is not None else None)
    torch.cuda.synchronize()
    _full_vs_slices("graph conv (bn1 stats)", _psum(rg), sums["g"], True)
    _full_vs_slices("temporal conv (bn2 stats)", _psum(ru), sums["u"], True)
    if kind == "conv":
        _full_vs_slices("residual conv (res_bn stats)", _psum(rr), sums["r"], True)

    # ---- float64 anchors, slice 0
    x0 = _back(s0["x"], cin, 2, T)
    ref = graph_ref(x0, eng.p[pre + "gcn.kernel"].cpu(), eng.p[pre + "gcn.bias"].cpu(), eng.A.cpu(), eng.tab_fwd)
    assert_bf16_close(_back(s0["gs"], f, 2, T), ref, "graph conv, slice 0")
    p = _psum(s0["r1"]).cpu()
    _slice_partials_close("graph conv", p[:, :1], ref.sum(dim=(0, 2, 3)).view(-1, 1), ref.abs().sum(dim=(0, 2, 3)))
    _slice_partials_close("graph conv (squares)", p[:, 1], (ref * ref).sum(dim=(0, 2, 3)))
    sc, sh = bn1.scale.cpu(), bn1.shift.cpu()
    gi = _back(s0["g_in"], f, 2, T)
    h = torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), gi.float(), sc.view(1, -1, 1, 1)))      # fp32 fma like the kernel
    ref = O.temporal_conv(_bf(h), _bf(eng.p[pre + "tcn.kernel"].cpu()), eng.p[pre + "tcn.bias"].cpu().double(), s)
    assert_bf16_close(_back(s0["us"], f, 2, To), ref, "temporal conv, slice 0")
    p = _psum(s0["r2"]).cpu()
    _slice_partials_close("temporal conv", p[:, :1], ref.sum(dim=(0, 2, 3)).view(-1, 1), ref.abs().sum(dim=(0, 2, 3)))
    _slice_partials_close("temporal conv (squares)", p[:, 1], (ref * ref).sum(dim=(0, 2, 3)))
    uref = _back(s0["us"], f, 2, To)
    z = uref * bn2.scale.cpu().double().view(1, -1, 1, 1) + bn2.shift.cpu().double().view(1, -1, 1, 1)
    if kind == "conv":
        ref = F.conv2d(x0, O.hwio_to_oihw(_bf(eng.p[pre + "res.kernel"].cpu())), eng.p[pre + "res.bias"].cpu().double(), stride=(s, 1))
        assert_bf16_close(_back(s0["rs"], f, 2, To), ref, "residual conv, slice 0")
        p = _psum(s0["r3"]).cpu()
        _slice_partials_close("residual conv", p[:, :1], ref.sum(dim=(0, 2, 3)).view(-1, 1), ref.abs().sum(dim=(0, 2, 3)))
        _slice_partials_close("residual conv (squares)", p[:, 1], (ref * ref).sum(dim=(0, 2, 3)))
        z = z + _back(s0["rs"], f, 2, To) * rbn.scale.cpu().double().view(1, -1, 1, 1) + rbn.shift.cpu().double().view(1, -1, 1, 1)
    elif kind == "identity":
        z = z + x0
    y0 = _back(_cols(y, To, 0), f, 2, To)
    assert_bf16_close(y0, torch.relu(z), "block tail, slice 0")
    m0 = _mask_bits(_cols(ym, To, 0), f).cpu()
    assert torch.equal(m0, (y0 > 0).permute(1, 0, 2, 3).reshape(f, -1)), "ReLU mask, slice 0"


# ----------------------------------------------------------------------------------------------------------------- 2. backward

@pytest.mark.parametrize("cin,f,s,T,blk", LAYERS)
def test_backward_at_bs64_equals_slices_and_float64(dev, eng, cin, f, s, T, blk):
    from sar_amd import ops8, stgcn8, _lib as L
    pre, kind = "l%d." % blk, eng.kinds[blk]
    conv, ident = kind == "conv", kind == "identity"
    To, pad = _same_pad(T, KT, s)
    n_in, n_out = B * T * V, B * To * V
    img = eng.packed.image
    bn1, bn2, rbn = eng.bn[pre + "bn1"], eng.bn[pre + "bn2"], eng.bn.get(pre + "res_bn")
    k = (bn2.k1, bn2.k2, bn2.k3)
    rk = (rbn.k1, rbn.k2, rbn.k3) if conv else None
    k1 = (bn1.k1, bn1.k2, bn1.k3)
    # stgcn8.backward: the graph data gradient gates block blk - 1's output gradient (SAR_EPI_ADD_GATE) unless that block has a
    # residual BatchNorm; it adds the skip-path gradient unless there is none (l0: no epilogue)
    assert stgcn8.FUSE_TAIL and stgcn8.RELU_MASK and eng.tab_bwd.g_flags & L.SAR_GRAPH_FEW_DENSE
    has_aux = kind != "none"
    gate = has_aux and blk >= 1 and eng.kinds[blk - 1] != "conv"
    print("l%d (%s): cin %d f %d stride %d T %d -> %d; graph data gradient epilogue %s" %
          (blk, kind, cin, f, s, T, To, "ADD_GATE" if gate else ("ADD" if has_aux else "NONE")))
    X = _rand8(cin, n_in, dev, 200 + blk)                 # block input
    G = _rand8(f, n_in, dev, 210 + blk)                   # graph conv output (pre-BN1)
    U = _rand8(f, n_out, dev, 220 + blk)                  # temporal conv output (pre-BN2)
    R = _rand8(f, n_out, dev, 230 + blk) if conv else None
    dY = _rand8(f, n_out, dev, 240 + blk)                 # output gradient of the block
    Y, YM = ops8.empty(f, n_out, dev), ops8.relu_mask(f, n_out, dev)
    ops8.bn_add_relu_fwd(U, bn2.scale, bn2.shift, {"none": 0, "identity": 1, "conv": 2}[kind], X if ident else R,
                         rbn.scale if conv else None, rbn.shift if conv else None, Y, f, mask=YM)
    if gate:
        Ub = _rand8(cin, n_in, dev, 250 + blk)            # block blk - 1's u and ReLU mask
        gen = torch.Generator(device=dev).manual_seed(260 + blk)
        MB = torch.randint(0, 256, ((cin + 7) // 8, n_in), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        mean_b = eng.bn["l%d.bn2" % (blk - 1)].mean

    def reduce(dy, y, u, r, m):
        return ops8.bn_add_relu_bwd_reduce(dy, y, u, r, f, bn2.mean, rbn.mean if conv else None, mask=m)

    def apply(dy, y, u, r, m, du, dr):
        """identity: dz written in place over a copy of dy, as stgcn8 writes it over dY.  Returns the gradient the skip path takes"""
        dz = dy.clone() if ident else None
        ops8.bn_add_relu_bwd_apply(dz if ident else dy, y, u, r, k, rk, du, dr, dz, f, mask=m)
        return dz

    def t_dgrad(du, g_, nb, out):
        return ops8.conv_gemm(L.SAR_CONV_TEMPORAL, du, out, img(pre + "tcn.b"), B=nb, V=V, T_src=To, T_out=T, Kc=f, M=f, taps=KT,
                              stride=s, pad=pad, transposed=True, epi=L.SAR_EPI_MASK, aux=g_, aux_affine=(bn1.scale, bn1.shift),
                              aux_mean=bn1.mean)

    def affine2(dz1, g_):
        dg = dz1.clone()
        ops8.affine2(dg, g_, k1, dg, f)                     # BN1 backward apply, in place as stgcn8 does
        return dg

    def r_dgrad(dr, nb, out):
        ops8.conv_gemm(L.SAR_CONV_TEMPORAL, dr, out, img(pre + "res.b"), B=nb, V=V, T_src=To, T_out=T, Kc=f, M=cin, taps=1,
                       stride=s, pad=0, transposed=True)

    def g_dgrad(dg, aux, nb, out, ub=None, mb=None):
        kw = dict(B=nb, V=V, T_src=T, T_out=T, Kc=f, M=cin, taps=KS, tables=eng.tab_bwd)
        if gate:
            return ops8.conv_gemm(L.SAR_CONV_GRAPH, dg, out, img(pre + "gcn.b"), epi=L.SAR_EPI_ADD_GATE, aux=aux, aux2=ub,
                                  aux_mask=mb, aux_mean=mean_b, **kw)
        return ops8.conv_gemm(L.SAR_CONV_GRAPH, dg, out, img(pre + "gcn.b"), epi=L.SAR_EPI_ADD if has_aux else L.SAR_EPI_NONE,
                              aux=aux, **kw)

    # ---- B = 128, in stgcn8._block_backward's order
    red = _poisoned(lambda: reduce(dY, Y, U, R, YM), [], dev)
    du, dr = ops8.empty(f, n_out, dev), (ops8.empty(f, n_out, dev) if conv else None)
    hold = {}
    _poisoned(lambda: hold.update(dz=apply(dY, Y, U, R, YM, du, dr)), [t for t in (du, dr) if t is not None], dev)
    dz = hold["dz"]
    dz1 = ops8.empty(f, n_in, dev)
    pm = _poisoned(lambda: t_dgrad(du, G, B, dz1), [dz1], dev)
    dg = affine2(dz1, G)
    dXres = None
    if conv:
        dXres = ops8.empty(cin, n_in, dev)
        _poisoned(lambda: r_dgrad(dr, B, dXres), [dXres], dev)
    aux = dz if ident else dXres
    dX = ops8.empty(cin, n_in, dev)
    pg = _poisoned(lambda: g_dgrad(dg, aux, B, dX, Ub if gate else None, MB if gate else None), [dX], dev)
    torch.cuda.synchronize()
    assert torch.isfinite(dX.float()).all() and torch.isfinite(dg.float()).all()

    # ---- the 64 slice launches
    acc_red = torch.zeros((f, 4), dtype=torch.float64, device=dev)
    acc_m = torch.zeros((f, 2), dtype=torch.float64, device=dev)
    acc_g = torch.zeros((cin, 2), dtype=torch.float64, device=dev)
    s0 = None
    for i in range(B // 2):
        dys, ys, us, ms = _cols(dY, To, i), _cols(Y, To, i), _cols(U, To, i), _cols(YM, To, i)
        rs = _cols(R, To, i) if conv else None
        rp = reduce(dys, ys, us, rs, ms)
        acc_red += _psum(rp)
        dus = _cols(du, To, i)
        dz1s = ops8.empty(f, 2 * T * V, dev)
        rm = t_dgrad(dus, _cols(G, T, i), 2, dz1s)
        acc_m += _psum(rm)
        dgs = _cols(dg, T, i)
        auxs = _cols(aux, T, i) if aux is not None else None
        dXs = ops8.empty(cin, 2 * T * V, dev)
        rg = g_dgrad(dgs, auxs, 2, dXs, _cols(Ub, T, i) if gate else None, _cols(MB, T, i) if gate else None)
        if gate:
            acc_g += _psum(rg)
        if i in SLICES:
            du_s, dr_s = ops8.empty(f, 2 * To * V, dev), (ops8.empty(f, 2 * To * V, dev) if conv else None)
            dz_s = apply(dys, ys, us, rs, ms, du_s, dr_s)
            assert torch.equal(du_s, dus), "bn_add_relu_bwd_apply du, slice %d" % i
            assert dr_s is None or torch.equal(dr_s, _cols(dr, To, i)), "bn_add_relu_bwd_apply dr, slice %d" % i
            assert dz_s is None or torch.equal(dz_s, _cols(dz, To, i)), "bn_add_relu_bwd_apply dz, slice %d" % i
            assert torch.equal(dz1s, _cols(dz1, T, i)), "temporal data gradient, slice %d" % i
            assert torch.equal(affine2(dz1s, _cols(G, T, i)), dgs), "affine2, slice %d" % i
            if conv:
                dXr_s = ops8.empty(cin, 2 * T * V, dev)
                r_dgrad(dr_s, 2, dXr_s)
                assert torch.equal(dXr_s, _cols(dXres, T, i)), "residual data gradient, slice %d" % i
            assert torch.equal(dXs, _cols(dX, T, i)), "graph data gradient, slice %d" % i
        if i == 0:
            s0 = dict(rp=rp, rm=rm, rg=rg, dX=dXs, dz1=dz1s)
    torch.cuda.synchronize()
    _full_vs_slices("bn_add_relu_bwd_reduce (mask)", _psum(red)[:, :3 if conv else 2], acc_red[:, :3 if conv else 2])
    _full_vs_slices("temporal data gradient (MASK sums)", _psum(pm), acc_m)
    if gate:
        _full_vs_slices("graph data gradient (ADD_GATE sums)", _psum(pg), acc_g)

    # ---- float64 anchors of the B = 128 BatchNorm-backward sums, from the stored bf16 tensors on the device
    dzf = _cn(dY, f) * _mask_bits(YM, f)
    terms = [dzf, dzf * (_cn(U, f) - bn2.mean.double().view(-1, 1))]
    if conv:
        terms.append(dzf * (_cn(R, f) - rbn.mean.double().view(-1, 1)))
    _anchor("bn_add_relu_bwd_reduce (mask)", _psum(red), terms)
    del terms
    dzs = _cn(dz1, f)
    gc = _cn(G, f) - bn1.mean.double().view(-1, 1)
    ul = _ulp(dzs)
    _anchor("temporal data gradient (MASK sums)", _psum(pm), [dzs, dzs * gc], ulps=[ul, ul * gc.abs()])
    del gc, ul
    if gate:
        dxs = _cn(dX, cin)
        _anchor("graph data gradient (ADD_GATE sums)", _psum(pg), [dxs, dxs * (_cn(Ub, cin) - mean_b.double().view(-1, 1))])
    del dzf, dzs

    # ---- float64 anchors, slice 0
    col = lambda t: t.cpu().double().view(-1, 1)
    cn0 = lambda t, C, Tt: ops8.to_cn(_cols(t, Tt, 0), C).cpu().double()
    dy0, u0, y0 = cn0(dY, f, To), cn0(U, f, To), cn0(Y, f, To)
    dz0 = dy0 * (y0 > 0)
    p = _psum(s0["rp"]).cpu()
    _slice_partials_close("bn_add_relu_bwd_reduce", p[:, :1], dz0.sum(dim=1).view(-1, 1), dz0.abs().sum(dim=1))
    _slice_partials_close("bn_add_relu_bwd_reduce (centred u)", p[:, 1], (dz0 * (u0 - col(bn2.mean))).sum(dim=1))
    assert_bf16_close(cn0(du, f, To), col(k[0]) * dz0 + col(k[1]) * u0 + col(k[2]), "bn_add_relu_bwd_apply du, slice 0")
    if conv:
        r0 = cn0(R, f, To)
        _slice_partials_close("bn_add_relu_bwd_reduce (centred r)", p[:, 2], (dz0 * (r0 - col(rbn.mean))).sum(dim=1))
        assert_bf16_close(cn0(dr, f, To), col(rk[0]) * dz0 + col(rk[1]) * r0 + col(rk[2]), "bn_add_relu_bwd_apply dr, slice 0")
    if ident:
        assert torch.equal(cn0(dz, f, To), dz0), "bn_add_relu_bwd_apply dz, slice 0"
    # temporal data gradient: transposed conv of the stored du with the bf16 weights, ReLU mask of the stored g through bn1
    du0 = _back(_cols(du, To, 0), f, 2, To)
    g0 = _back(_cols(G, T, 0), f, 2, T)
    hh = torch.zeros(2, f, T, V, dtype=torch.float64, requires_grad=True)
    dh, = torch.autograd.grad(O.temporal_conv(hh, _bf(eng.p[pre + "tcn.kernel"].cpu()), None, s), hh, du0)
    pre_act = torch.addcmul(bn1.shift.cpu().view(1, -1, 1, 1), g0.float(), bn1.scale.cpu().view(1, -1, 1, 1))
    g_pre = dh * (pre_act > 0)
    dz1_0 = _back(s0["dz1"], f, 2, T)
    assert_bf16_close(dz1_0, g_pre, "temporal data gradient, slice 0")
    p = _psum(s0["rm"]).cpu()
    _slice_partials_close("temporal data gradient", p[:, :1], g_pre.sum(dim=(0, 2, 3)).view(-1, 1), g_pre.abs().sum(dim=(0, 2, 3)))
    _slice_partials_close("temporal data gradient (centred)", p[:, 1],
                          (g_pre * (g0 - bn1.mean.cpu().double().view(1, -1, 1, 1))).sum(dim=(0, 2, 3)))
    c4 = lambda t: t.cpu().double().view(1, -1, 1, 1)
    dg0 = _back(_cols(dg, T, 0), f, 2, T)
    assert_bf16_close(dg0, c4(k1[0]) * dz1_0 + c4(k1[1]) * g0 + c4(k1[2]), "affine2, slice 0")
    add0 = None
    if conv:
        dr0 = _back(_cols(dr, To, 0), f, 2, To)
        xx = torch.zeros(2, cin, T, V, dtype=torch.float64, requires_grad=True)
        yy = F.conv2d(xx, O.hwio_to_oihw(_bf(eng.p[pre + "res.kernel"].cpu())), None, stride=(s, 1))
        gx, = torch.autograd.grad(yy, xx, dr0)
        add0 = _back(_cols(dXres, T, 0), cin, 2, T)
        assert_bf16_close(add0, gx, "residual data gradient, slice 0")
    elif ident:
        add0 = _back(_cols(dz, T, 0), cin, 2, T)
    kern = eng.p[pre + "gcn.kernel"].cpu()
    kT = kern[0, 0].view(cin, KS, f).permute(2, 1, 0).reshape(1, 1, f, KS * cin)      # [m][k*cin + c]
    ref = graph_ref(dg0, kT, None, None, eng.tab_bwd)
    if add0 is not None:
        ref = ref + add0
    if gate:
        keep = _mask_bits(_cols(MB, T, 0), cin).cpu().view(cin, 2, T, V).permute(1, 0, 2, 3)
        ref = torch.where(keep, ref, torch.zeros((), dtype=torch.float64))
    dX0 = _back(s0["dX"], cin, 2, T)
    assert_bf16_close(dX0, ref, "graph data gradient, slice 0")
    if gate:
        # the gated sums run over the STORED output (test_gpu_cn8.test_graph_data_gradient_gated_epilogue)
        p = _psum(s0["rg"]).cpu()
        ub0 = _back(_cols(Ub, T, 0), cin, 2, T)
        s1 = dX0.sum(dim=(0, 2, 3))
        s2 = (dX0 * (ub0 - mean_b.cpu().double().view(1, -1, 1, 1))).sum(dim=(0, 2, 3))
        _slice_partials_close("graph data gradient (ADD_GATE sums)", p[:, :1], s1.view(-1, 1), dX0.abs().sum(dim=(0, 2, 3)))
        _slice_partials_close("graph data gradient (ADD_GATE centred)", p[:, 1:], s2.view(-1, 1),
                              (dX0 * (ub0 - mean_b.cpu().double().view(1, -1, 1, 1))).abs().sum(dim=(0, 2, 3)))


# ----------------------------------------------------------------------------------------------------------------- 3. weight gradients

def _wgrad_split(mode, nb, T_out, Kc, M, taps):
    """(ntiles, nsplit, tiles per split, splits without a tile) by ops8.conv_wgrad's formula and the kernel's tile map
    (csrc/conv_wgrad_cn8.hip: split i takes tiles [i tps, min((i + 1) tps, ntiles)))"""
    from sar_amd import ops8, _lib as L
    ft = L.load().sar_conv_wgrad_cn8_tile_frames(mode)
    ntiles = nb * ((T_out + ft - 1) // ft)
    cb = 32 if (mode == L.SAR_CONV_TEMPORAL and taps == 9) else 64
    blocks = ((M + 63) // 64) * ((Kc + cb - 1) // cb)
    nsplit = max(1, min(ntiles, (ops8._WGRAD_SLOTS + blocks - 1) // blocks))
    tps = (ntiles + nsplit - 1) // nsplit
    return ntiles, nsplit, tps, nsplit - (ntiles + tps - 1) // tps


def _wgrad_launches(eng, cin, f, s, T, blk):
    """(name, mode, Kc, M, taps, T_out, flat slice of eng.grad, wsize, bsize, kwargs) of the block's weight gradients, as stgcn8"""
    from sar_amd import _lib as L
    pre = "l%d." % blk
    To, pad = _same_pad(T, KT, s)
    bn1 = eng.bn[pre + "bn1"]
    o = eng.offsets
    out = [("temporal 9-tap", L.SAR_CONV_TEMPORAL, f, f, KT, To, eng.grad[o[pre + "tcn.kernel"]:o[pre + "tcn.bias"] + f], KT * f * f, f,
            dict(stride=s, pad=pad, pro=(bn1.scale, bn1.shift), pro_relu=True, w_stride_tap=f * f, w_stride_c=f)),
           ("graph", L.SAR_CONV_GRAPH, cin, f, KS, T, eng.grad[o[pre + "gcn.kernel"]:o[pre + "gcn.bias"] + KS * f], cin * KS * f, KS * f,
            dict(tables=eng.tab_fwd, w_stride_tap=f, w_stride_c=KS * f))]
    if eng.kinds[blk] == "conv":
        out.append(("residual 1-tap", L.SAR_CONV_TEMPORAL, cin, f, 1, To, eng.grad[o[pre + "res.kernel"]:o[pre + "res.bias"] + f], cin * f, f,
                    dict(stride=s, pad=0, w_stride_tap=0, w_stride_c=f)))
    return out


def test_wgrad_split_table_has_empty_splits(dev, eng):
    """the regime of section 3 that only the bench batch reaches: splits of the B = 128 weight gradients that get no tile and
    must still write a zero row into the engine's persistent slab.  Asserted to exist so that it cannot disappear silently."""
    empty = []
    print("block  launch           B = 128: ntiles  nsplit  tps  empty     B = 2: ntiles  nsplit  tps  empty")
    for cin, f, s, T, blk in LAYERS:
        for name, mode, Kc, M, taps, T_out, *_ in _wgrad_launches(eng, cin, f, s, T, blk):
            row = _wgrad_split(mode, B, T_out, Kc, M, taps)
            print("l%-5d %-16s %15d  %6d  %3d  %5d  %13d  %6d  %3d  %5d" % (blk, name, *row, *_wgrad_split(mode, 2, T_out, Kc, M, taps)))
            if row[3]:
                empty.append(("l%d" % blk, name))
    print("launches with empty splits:", empty)
    assert empty


@pytest.mark.parametrize("cin,f,s,T,blk", LAYERS)
def test_weight_gradients_at_bs64_through_poisoned_slabs(dev, eng, cin, f, s, T, blk):
    from sar_amd import ops, ops8
    To, pad = _same_pad(T, KT, s)
    n_in, n_out = B * T * V, B * To * V
    slabs = eng._slabs
    assert slabs is not None
    G = _rand8(f, n_in, dev, 300 + blk)                   # temporal conv input (pre-BN1)
    dU = _rand8(f, n_out, dev, 310 + blk)
    X = _rand8(cin, n_in, dev, 320 + blk)
    dG = _rand8(f, n_in, dev, 330 + blk)
    dR = _rand8(f, n_out, dev, 340 + blk)
    operands = {"temporal 9-tap": (G, dU, T), "graph": (X, dG, T), "residual 1-tap": (X, dR, T)}
    launches = _wgrad_launches(eng, cin, f, s, T, blk)
    for name, mode, Kc, M, taps, T_out, flat, wsize, bsize, kw in launches:
        src, dout, Ts = operands[name]
        ntiles, nsplit, tps, empty = _wgrad_split(mode, B, T_out, Kc, M, taps)
        print("l%d %s: ntiles %d nsplit %d tps %d empty splits %d" % (blk, name, ntiles, nsplit, tps, empty))
        slab = slabs.slab(flat, nsplit, wsize + bsize)
        slab.fill_(float("nan"))
        flat.fill_(float("nan"))
        ops8.conv_wgrad(mode, src, dout, flat, B=B, V=V, T_src=Ts, T_out=T_out, Kc=Kc, M=M, taps=taps, wsize=wsize, bsize=bsize,
                        slabs=slabs, **kw)
        assert slabs._pending[-1][0] == slab.data_ptr() and slabs._pending[-1][4] == nsplit, "the launch did not take the poisoned slab"
    slabs.flush()
    torch.cuda.synchronize()
    fulls = {ln[0]: ln[6].clone() for ln in launches}
    acc = {ln[0]: torch.zeros(ln[7] + ln[8], dtype=torch.float64, device=dev) for ln in launches}
    # the slices through a SlabBatch of their own, NaN-filled slabs too: at B = 2 the 9-tap launches of l7 / l8 have empty splits
    sb, outs, first = ops.SlabBatch(), {ln[0]: torch.empty(ln[7] + ln[8], device=dev) for ln in launches}, {}
    for i in range(B // 2):
        for name, mode, Kc, M, taps, T_out, flat, wsize, bsize, kw in launches:
            src, dout, Ts = operands[name]
            out = outs[name]
            out.fill_(float("nan"))
            sb.slab(out, _wgrad_split(mode, 2, T_out, Kc, M, taps)[1], wsize + bsize).fill_(float("nan"))
            ops8.conv_wgrad(mode, _cols(src, Ts, i), _cols(dout, T_out, i), out, B=2, V=V, T_src=Ts, T_out=T_out, Kc=Kc, M=M, taps=taps,
                            wsize=wsize, bsize=bsize, slabs=sb, **kw)
        sb.flush()
        for name, *_ in launches:
            acc[name] += outs[name].double()
            if i == 0:
                first[name] = outs[name].clone()
    assert len(sb._slabs) == len(launches)          # every slice launch took the slab filled above
    torch.cuda.synchronize()
    for name, mode, Kc, M, taps, T_out, flat, wsize, bsize, kw in launches:
        full = fulls[name]
        assert torch.isfinite(full).all(), "%s: non-finite weight gradient (a slab row left unwritten)" % name
        ew, eb = rel_err(full[:wsize], acc[name][:wsize]), rel_err(full[wsize:], acc[name][wsize:])
        print("l%d %s: B=128 launch through the poisoned slab vs float64 sum of the 64 slice launches: dW %.2e, dbias %.2e" %
              (blk, name, ew, eb))
        assert ew < RED_TOL and eb < RED_TOL, name

    # ---- float64 anchors, slice 0
    pre = "l%d." % blk
    bn1 = eng.bn[pre + "bn1"]
    g0, du0 = _back(_cols(G, T, 0), f, 2, T), _back(_cols(dU, To, 0), f, 2, To)
    h = _bf(torch.relu(torch.addcmul(bn1.shift.cpu().view(1, -1, 1, 1), g0.float(), bn1.scale.cpu().view(1, -1, 1, 1))))
    kernel = torch.zeros(KT, 1, f, f, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(f, dtype=torch.float64, requires_grad=True)
    gk, gb = torch.autograd.grad(O.temporal_conv(h, kernel, bias, s), (kernel, bias), du0)
    w = first["temporal 9-tap"].cpu()
    _wgrad_anchor(blk, "temporal 9-tap", w[:KT * f * f].view(KT, 1, f, f), gk, w[KT * f * f:], gb)
    x0, dg0 = _back(_cols(X, T, 0), cin, 2, T), _back(_cols(dG, T, 0), f, 2, T)
    tab = eng.tab_fwd
    idx, wt = tab.idx.cpu(), tab.wt.cpu()
    xs = x0.float()
    gk = torch.zeros(cin, KS * f, dtype=torch.float64)
    gb = torch.zeros(KS * f, dtype=torch.float64)
    A = eng.A.cpu()
    for kk in range(KS):
        z = torch.zeros(2, cin, T, V)
        for v in range(V):
            a = wt[kk, v, 0] * xs[:, :, :, idx[kk, v, 0]]
            for j in range(1, tab.nz[kk]):
                a = torch.addcmul(a, xs[:, :, :, idx[kk, v, j]], wt[kk, v, j])          # fp32 fma chain, table order
            z[:, :, :, v] = a
        gk[:, kk * f:(kk + 1) * f] = torch.einsum("bctv,bmtv->cm", _bf(z), dg0)
        gb[kk * f:(kk + 1) * f] = torch.einsum("bmtv,v->m", dg0, A[kk].double().sum(dim=0))
    w = first["graph"].cpu()
    _wgrad_anchor(blk, "graph", w[:cin * KS * f].view(cin, KS * f), gk, w[cin * KS * f:], gb)
    if eng.kinds[blk] == "conv":
        dr0 = _back(_cols(dR, To, 0), f, 2, To)
        kernel = torch.zeros(1, 1, cin, f, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(f, dtype=torch.float64, requires_grad=True)
        yy = F.conv2d(x0, O.hwio_to_oihw(kernel), bias, stride=(s, 1))
        gk, gb = torch.autograd.grad(yy, (kernel, bias), dr0)
        w = first["residual 1-tap"].cpu()
        _wgrad_anchor(blk, "residual 1-tap", w[:cin * f].view(1, 1, cin, f), gk, w[cin * f:], gb)


def _wgrad_anchor(blk, name, w, gk, b, gb):
    ew, eb = rel_err(w, gk), rel_err(b, gb)
    print("l%d %s: slice 0 vs float64 definition: dW %.2e, dbias %.2e" % (blk, name, ew, eb))
    assert ew < 1e-5 and eb < 1e-5, name


# ----------------------------------------------------------------------------------------------------------------- 5. engine

@pytest.mark.parametrize("classes,stream", [(60, "joint"), (120, "bone")])
def test_bf16_eval_logits_bs64_equal_chunks(dev, classes, stream):
    """The bf16 engine, all 10 blocks, T = 300, bs = 64, inference (moving statistics): every clip's logits are independent of
    its batch-mates, so bs = 64 must reproduce 2-clip forwards bit for bit (data_bn_apply and pool_fwd in CN8 included)."""
    from sar_amd.bone import NTU_BONE_PAIRS
    from sar_amd.stgcn import STGCN
    from sar_amd.train import synthetic_clips
    eng = STGCN(num_classes=classes, device=dev, seed=3, mfma="bf16", bone_pairs=NTU_BONE_PAIRS if stream == "bone" else None)
    g = torch.Generator(device=dev).manual_seed(5)
    for name, bn in eng.bn.items():               # non-trivial moving statistics
        bn.moving_mean.copy_(0.1 * torch.randn(bn.moving_mean.shape, generator=g, device=dev))
        bn.moving_var.copy_(1 + 0.3 * torch.rand(bn.moving_var.shape, generator=g, device=dev))
    x, _ = synthetic_clips(64, dev, seed=9, num_classes=classes)
    full = eng.forward(x, training=False).clone()
    torch.cuda.synchronize()
    assert full.shape == (64, classes) and torch.isfinite(full).all() and full.std() > 0
    for i in (0, 1, 15, 31):
        part = eng.forward(x[2 * i:2 * i + 2].contiguous(), training=False)
        assert torch.equal(part, full[2 * i:2 * i + 2]), "clips %d-%d" % (2 * i, 2 * i + 1)
    print("bf16 eval logits, %s / %d classes: clips 0-1, 2-3, 30-31, 62-63 equal 2-clip forwards (logit std %.3f)" %
          (stream, classes, full.std().item()))
