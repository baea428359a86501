"""Tensor-level wrappers of the bf16 configuration's kernels (include/sar_hip.h, "CN8" section; csrc/cn8.h).

A CN8 activation is a torch.bfloat16 tensor of shape (G, ld, 8): G = ceil(C/8) planes of ld 16-byte units, unit
(g, col) = channels 8g..8g+7 of column col = (b*T + t)*V + v.  torch is used for device memory and the stream only.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from . import profiler
from ._lib import check, ptr, stream_ptr
from .ops import _REDUCING, _conv_desc, _data_bn_dx_out, _reducing_partials, _wgrad_desc, _wgrad_slab, _wgrad_slab_done

_MFMA_GATHER = os.environ.get("SAR_CN8_MFMA_GATHER", "1") == "1"   # A/B switch: 0 keeps the vector-ALU gather of the dense adjacency slice


def empty(channels, n, device):
    return torch.empty(((channels + 7) // 8, n, 8), dtype=torch.bfloat16, device=device)


def _cn8(t):
    assert t is None or (t.dtype == torch.bfloat16 and t.is_cuda and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 8), \
        "need a contiguous cuda CN8 tensor (G, ld, 8) of bfloat16"
    return t


def _f32(t):
    assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()), "need contiguous cuda float32"
    return t


def _rows(t):
    """an fp32 CN matrix, possibly a view of rows with a leading dimension stride(0) >= n (the fp32 `ld` contract)"""
    assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), "need cuda float32 rows"
    return t


def from_cn(x, out=None):
    """fp32 CN matrix [C][n] (row stride ld_x >= n) -> CN8 (rounded to bfloat16, nearest even).  out: a CN8 tensor (G, ld_out >= n, 8)
    whose first n units per plane are written"""
    Cc, n = x.shape
    if out is None:
        out = empty(Cc, n, x.device)
    assert _cn8(out).shape[0] == (Cc + 7) // 8
    check(L.load().sar_cn_to_cn8(ptr(_rows(x)), x.stride(0), ptr(out), out.shape[1], Cc, n, stream_ptr()), "sar_cn_to_cn8")
    return out


def to_cn(x8, channels, n=None, out=None):
    """CN8 -> fp32 CN matrix [channels][n].  n: the live width (default: ld = x8.shape[1]); out: fp32 rows of stride ld_out >= n"""
    n = x8.shape[1] if n is None else n
    if out is None:
        out = torch.empty((channels, n), dtype=torch.float32, device=x8.device)
    assert tuple(out.shape) == (channels, n)
    check(L.load().sar_cn8_to_cn(ptr(_cn8(x8)), x8.shape[1], ptr(_rows(out)), out.stride(0), channels, n, stream_ptr()), "sar_cn8_to_cn")
    return out


_CN8 = (lambda t: (ptr(_cn8(t)), t.shape[1]), _f32)      # a CN8 operand -> (pointer, leading dimension in units); a per-channel vector


def conv_gemm(mode, src, out, packed, *, B, V, T_src, T_out, Kc, M, taps, stride=1, pad=0, transposed=False, bias=None,
              pro=None, pro_relu=False, tables=None, epi=L.SAR_EPI_NONE, aux=None, aux_affine=None, aux_mean=None, aux2=None,
              aux_mask=None):
    """sar_conv_gemm_cn8: src / out / aux CN8, `packed` the bf16 weight image (ops.PackedWeights.image).  Returns
    (partials, nparts) when the epilogue reduces.  SAR_EPI_ADD_GATE (graph data gradient): out = gate(acc + aux) with the gate
    bytes `aux_mask`, partial sums (sum out, sum out (aux2 - aux_mean))."""
    lib = L.load()
    _cn8(src), _cn8(out), _cn8(aux)
    assert src.shape[0] == (Kc + 7) // 8 and out.shape[0] == (M + 7) // 8 and (aux is None or aux.shape[0] == out.shape[0])
    d = _conv_desc(_CN8, mode, src, out, B, V, T_src, T_out, Kc, M, taps, stride, pad, transposed, epi, pro, pro_relu, tables,
                   getattr(tables, "g_flags", 0) if _MFMA_GATHER else 0, bias, aux, aux_affine, aux_mean)
    if epi == L.SAR_EPI_ADD_GATE:
        assert aux2 is not None and aux_mask is not None and aux_mean is not None and aux2.shape[0] == out.shape[0]
        assert aux_mask.dtype == torch.uint8 and aux_mask.shape == (out.shape[0], aux2.shape[1]) and aux_mask.is_contiguous()
        _cn8(aux2)
        d.aux2, d.ld_aux2, d.aux_mask = ptr(aux2), aux2.shape[1], ptr(aux_mask)
    partials, nparts = None, 0
    if epi in _REDUCING:
        nparts = lib.sar_conv_gemm_cn8_nparts(C.byref(d))
        partials = _reducing_partials(d, nparts, "sar_conv_gemm_cn8_nparts", M, src.device)
    n_conv = B * (T_src if transposed else T_out) * V
    tag = ("gemm_graph" if mode == L.SAR_CONV_GRAPH else ("gemm_temporal%d%s" % (taps, "_dgrad" if transposed else ""))) + "_cn8"
    with profiler.region(tag, 2.0 * M * Kc * taps * n_conv, 2.0 * (Kc * B * T_src * V + M * B * T_out * V)):
        check(lib.sar_conv_gemm_cn8(C.byref(d), ptr(packed), stream_ptr()), "sar_conv_gemm_cn8")
    return (partials, nparts) if partials is not None else None


_WGRAD_SLOTS = int(os.environ.get("SAR_WGRAD8_SLOTS", "512"))


def conv_wgrad(mode, src, dout, dW_out, *, B, V, T_src, T_out, Kc, M, taps, stride=1, pad=0, pro=None, pro_relu=False,
               tables=None, w_stride_tap, w_stride_c, wsize, bsize, nsplit=None, slabs=None):
    """sar_conv_wgrad_cn8 + sar_slab_reduce_f32: dW (and dbias right behind it) -> dW_out[0 : wsize + bsize] (flat fp32).
    slabs (ops.SlabBatch): the slabs are summed by the batch's next flush() instead of by a launch of their own."""
    lib = L.load()
    d = _wgrad_desc(_CN8, mode, src, dout, B, V, T_src, T_out, Kc, M, taps, stride, pad, pro, pro_relu, tables,
                    getattr(tables, "g_flags", 0) if _MFMA_GATHER else 0, w_stride_tap, w_stride_c, wsize, bsize)
    if nsplit is None:           # two resident workgroups per CU (SAR_WGRAD8_SLOTS: sweep knob, tools)
        ft = lib.sar_conv_wgrad_cn8_tile_frames(mode)
        ntiles = B * ((T_out + ft - 1) // ft)
        cb = 32 if (mode == L.SAR_CONV_TEMPORAL and taps == 9) else 64
        blocks = ((M + 63) // 64) * ((Kc + cb - 1) // cb)
        nsplit = max(1, min(ntiles, (_WGRAD_SLOTS + blocks - 1) // blocks))
    ident, n = (int(getattr(tables, "slice0_identity", False)) if tables is not None else 0), wsize + bsize
    slab = _wgrad_slab(d, slabs, dW_out, nsplit, n, src.device)
    tag = ("wgrad_graph" if mode == L.SAR_CONV_GRAPH else "wgrad_temporal%d" % taps) + "_cn8"
    with profiler.region(tag, 2.0 * M * Kc * taps * B * T_out * V, 2.0 * (Kc * B * T_src * V + M * B * T_out * V)):
        check(lib.sar_conv_wgrad_cn8(C.byref(d), ident, stream_ptr()), "sar_conv_wgrad_cn8")
    _wgrad_slab_done(slabs, slab, nsplit, n, dW_out)


def relu_mask(channels, n, device):
    """one byte per unit: the ReLU mask of a block tail's output (the mask of sar_bn_add_relu_fwd_cn8)"""
    return torch.empty(((channels + 7) // 8, n), dtype=torch.uint8, device=device)


def bn_add_relu_fwd(u, sc, sh, res_kind, r, rsc, rsh, y, channels, mask=None, n=None):
    """n: the live width (default: ld = u.shape[1]; every tensor, and the mask, has u's ld)"""
    n = u.shape[1] if n is None else n
    check(L.load().sar_bn_add_relu_fwd_cn8(ptr(_cn8(u)), ptr(sc), ptr(sh), res_kind, ptr(_cn8(r)), ptr(rsc), ptr(rsh), ptr(_cn8(y)),
                                           ptr(mask), channels, n, u.shape[1], stream_ptr()), "sar_bn_add_relu_fwd_cn8")


_REDUCE_CHUNK = int(os.environ.get("SAR_BWD_REDUCE_CHUNK8", "8192"))     # units per workgroup of the BN-backward reduction


def bn_add_relu_bwd_reduce(dy, y, u, r, channels, mu=None, mr=None, tail=None, mask=None, n=None):
    """mask (relu_mask written by bn_add_relu_fwd): read instead of y.  n: the live width (default: ld = u.shape[1])"""
    ld = u.shape[1]
    n = ld if n is None else n
    nparts = max(1, min(4096, (n + _REDUCE_CHUNK - 1) // _REDUCE_CHUNK))
    partials = torch.empty((channels, nparts, 4), dtype=torch.float32, device=u.device)
    # tail (ops.make_bn_tail): the last workgroup of every plane finalises its channels; this layout has never combined it with a mask
    assert mask is None or tail is None
    check(L.load().sar_bn_add_relu_bwd_reduce_cn8(ptr(_cn8(dy)), ptr(_cn8(y)), ptr(mask), ptr(_cn8(u)), ptr(_cn8(r)), ptr(mu), ptr(mr),
                                                  ptr(partials), nparts, channels, n, ld,
                                                  C.byref(tail) if tail is not None else None, stream_ptr()),
          "sar_bn_add_relu_bwd_reduce_cn8")
    return partials, nparts


def bn_add_relu_bwd_apply(dy, y, u, r, k, rk, du, dr, dz_out, channels, mask=None, n=None):
    """n: the live width (default: ld = u.shape[1])"""
    rk = rk or (None, None, None)
    ld = u.shape[1]
    n = ld if n is None else n
    check(L.load().sar_bn_add_relu_bwd_apply_cn8(ptr(_cn8(dy)), ptr(_cn8(y)), ptr(mask), ptr(_cn8(u)), ptr(_cn8(r)), ptr(k[0]), ptr(k[1]),
                                                 ptr(k[2]), ptr(rk[0]), ptr(rk[1]), ptr(rk[2]), ptr(_cn8(du)), ptr(_cn8(dr)),
                                                 ptr(_cn8(dz_out)), channels, n, ld, stream_ptr()), "sar_bn_add_relu_bwd_apply_cn8")


def affine2(a, b, k, out, channels, n=None):
    """n: the live width (default: ld = a.shape[1])"""
    ld = a.shape[1]
    n = ld if n is None else n
    check(L.load().sar_affine2_cn8(ptr(_cn8(a)), ptr(_cn8(b)), ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(_cn8(out)), channels, n, ld,
                                   stream_ptr()), "sar_affine2_cn8")


def data_bn_apply(x, bone_parent, scale, shift, out, motion=False):
    N, C_, T, V, M = x.shape
    check(L.load().sar_data_bn_apply_cn8(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(scale), ptr(shift),
                                         ptr(_cn8(out)), out.shape[1], stream_ptr()), "sar_data_bn_apply_cn8")


def data_bn_bwd_reduce(x, bone_parent, dy, mean, partials, motion=False):
    N, C_, T, V, M = x.shape
    check(L.load().sar_data_bn_bwd_reduce_cn8(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(_cn8(dy)), dy.shape[1],
                                              ptr(mean), ptr(partials), stream_ptr()), "sar_data_bn_bwd_reduce_cn8")


def data_bn_bwd_apply(x, bone_parent, dy, k, dx=None, motion=False):
    """ops.data_bn_bwd_apply with dy = the (C <= 8)-channel CN8 plane; dx is float32 (N, C, T, V, M)"""
    dx = _data_bn_dx_out(x, dx)
    N, C_, T, V, M = x.shape
    check(L.load().sar_data_bn_bwd_apply_cn8(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(_cn8(dy)), dy.shape[1],
                                             ptr(_f32(k[0])), ptr(_f32(k[1])), ptr(_f32(k[2])), ptr(dx), stream_ptr()),
          "sar_data_bn_bwd_apply_cn8")
    return dx


def pool_fwd(y, channels, B, TV, Mp, feat):
    check(L.load().sar_pool_fwd_cn8(ptr(_cn8(y)), y.shape[1], channels, B, TV, Mp, ptr(feat), stream_ptr()), "sar_pool_fwd_cn8")


def pool_bwd(dfeat, channels, B, TV, Mp, dy):
    check(L.load().sar_pool_bwd_cn8(ptr(dfeat), dy.shape[1], channels, B, TV, Mp, ptr(_cn8(dy)), stream_ptr()), "sar_pool_bwd_cn8")
