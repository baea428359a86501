"""Thin tensor-level wrappers over the C ABI (include/sar_hip.h).  torch is used only for device
memory and the current HIP stream; all arithmetic happens in libsar_hip.so.

Activations use the CN layout: a 2-D float32 tensor [C][B*T*V] (see include/sar_hip.h).
"""
import ctypes as C
import os

import torch

from . import _lib as L
from . import operands as O
from . import profiler
from ._lib import ConvDesc, WgradDesc, check, ptr, stream_ptr


_PROFILE_SHAPES = os.environ.get("SAR_PROFILE_SHAPES", "0") == "1"


def _f32(t):
    # a 2-D operand may be a row-strided view (unit column stride, ld = stride(0) >= the row length): the ABI takes every `ld`
    assert t is None or (t.dtype == torch.float32 and t.is_cuda and
                         (t.is_contiguous() or (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]))), \
        "need cuda float32, contiguous or a 2-D view with unit column stride"
    return t


class GraphTables:
    """Device copies of the gather lists (graph_tables.gather_lists)."""

    def __init__(self, A, device, transpose=False):
        from .graph_tables import gather_lists
        idx, wt, nz, colsum = gather_lists(A, transpose)
        self.idx = torch.from_numpy(idx).to(device)
        self.wt = torch.from_numpy(wt).to(device)
        self.colsum = torch.from_numpy(colsum).to(device)
        self.nz = nz
        self.K, self.V = idx.shape[0], idx.shape[1]
        # slice 0 is the identity (the 'spatial' strategy's self-links, graph/tools.py:22-30): gather list {(v, 1.0)}
        import numpy as np
        self.slice0_identity = bool(nz[0] == 1 and np.array_equal(idx[0, :, 0], np.arange(self.V)) and np.all(wt[0, :, 0] == 1.0))
        # every gather weight exactly representable in bfloat16 (NTU: 0.25 / 0.5 / 1): the CN8 kernels may then apply a dense
        # slice on the matrix cores (SAR_GRAPH_WT_BF16_EXACT, include/sar_hip.h)
        w32 = torch.from_numpy(np.ascontiguousarray(wt, dtype=np.float32))
        self.g_flags = L.SAR_GRAPH_WT_BF16_EXACT if bool(torch.equal(w32.to(torch.bfloat16).to(torch.float32), w32)) else 0
        # gather lists that are neither {one entry of weight 1} nor empty: the CN8 graph convolution builds only those and reads
        # every other operand straight from the raw tile (SAR_GRAPH_FEW_DENSE, csrc/conv_graph_cn8.hip)
        wnp = np.asarray(wt, dtype=np.float32)
        cnt = (wnp != 0).sum(axis=2)
        first = np.take_along_axis(wnp, np.argmax(wnp != 0, axis=2)[..., None], axis=2)[..., 0]
        self.n_dense_lists = int(((cnt > 1) | ((cnt == 1) & (first != 1.0))).sum())
        if self.slice0_identity:
            self.g_flags |= L.SAR_GRAPH_SLICE0_IDENTITY
        # (<= 12: what the read-gather kernels hold as virtual joints of a V = 25 tile -- conv_graph_cn8.hip needs 2 FT nv <= 256 --;
        # denser tables keep the unit-builder / fp32 kernels and the unfused block tail)
        if self.n_dense_lists <= 12:
            self.g_flags |= L.SAR_GRAPH_FEW_DENSE | (self.n_dense_lists << L.SAR_GRAPH_FEW_DENSE_SHIFT)


class PackedWeights:
    """bf16 operand images of many weight tensors, refreshed from the flat parameter buffer by ONE launch
    (sar_pack_weights_bf16_batch).  add() registers element (tap, c, m) at base[src_off + tap*st + c*sc + m*sm]; a data
    gradient registers the same tensor with the roles of c and m exchanged (no transposed copy)."""

    ITEM = [("src_off", "<i8"), ("st", "<i8"), ("sc", "<i8"), ("sm", "<i8"), ("dst_unit", "<i8"),
            ("taps", "<i4"), ("Kc", "<i4"), ("M", "<i4"), ("G", "<i4")]

    def __init__(self):
        self.items, self.index, self.units = [], {}, 0

    def add(self, key, src_off, st, sc, sm, taps, Kc, M):
        G = 2 * ((Kc + 15) // 16)
        n = taps * G * M
        self.index[key] = (self.units, n)
        self.items.append((src_off, st, sc, sm, self.units, taps, Kc, M, G))
        self.units += n

    def finalize(self, device):
        import numpy as np
        tab = np.array(self.items, dtype=np.dtype(self.ITEM, align=True))
        assert tab.dtype.itemsize == 56          # sizeof(sar_pack_item)
        self.table = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(device)
        self.max_units = max(it[5] * it[8] * it[7] for it in self.items)
        self.buf = torch.empty(self.units * 16, dtype=torch.uint8, device=device)

    def refresh(self, flat):
        check(L.load().sar_pack_weights_bf16_batch(ptr(flat), ptr(self.table), len(self.items), self.max_units, ptr(self.buf),
                                                   stream_ptr()), "sar_pack_weights_bf16_batch")

    def image(self, key):
        off, n = self.index[key]
        return self.buf[off * 16:(off + n) * 16]


class PackedSplitWeights(PackedWeights):
    """Term images of many weight tensors for the split-arithmetic kernels (sar_conv_gemm_split, include/sar_hip.h): the same
    items as PackedWeights with channel groups of 8 and `terms` images per item, refreshed by ONE call per step; the fp16
    arithmetics also get every item's amax (the bits of a float, device memory) = its `w_bound`."""

    TERMS = {"bf16x1": 1, "bf16x3": 2, "bf16x6": 3, "bf16x9": 3, "f16x3": 2, "f16x3s": 2, "f16x3a": 3}

    def __init__(self, arith):
        super().__init__()
        self.arith, self.terms, self.item_of = arith, self.TERMS[arith], {}

    def add(self, key, src_off, st, sc, sm, taps, Kc, M):
        G = (Kc + 7) // 8
        n = self.terms * taps * G * M
        self.index[key] = (self.units, n)
        self.item_of[key] = len(self.items)
        self.items.append((src_off, st, sc, sm, self.units, taps, Kc, M, G))
        self.units += n

    def finalize(self, device):
        super().finalize(device)
        self.amax = torch.zeros(len(self.items), dtype=torch.int32, device=device)

    def refresh(self, flat):
        check(L.load().sar_pack_weights_split_batch(ptr(flat), ptr(self.table), len(self.items), self.max_units,
                                                    L.SAR_SPLIT[self.arith], ptr(self.buf), ptr(self.amax), stream_ptr()),
              "sar_pack_weights_split_batch")

    def bound(self, key):
        i = self.item_of[key]
        return self.amax[i:i + 1]


_WGRADS_SLOTS = int(os.environ.get("SAR_WGRAD_SPLIT_SLOTS", "512"))   # workgroups of a split weight-gradient launch (default: two per CU)
_side_streams = {}
GRAPH_ONE_TILE_WG = False     # tests / A-B: the round-5 graph kernel of the split arithmetic (include/sar_hip.h: SAR_GRAPH_ONE_TILE_WG)
SIDE_CU_MASK_DEFAULT = "off"


def shared_side_stream(device, priority=0):
    """ONE weight-gradient stream per (device, host thread, priority) for every engine of the process.  HIP maps streams onto a few
    hardware queues round-robin in creation order: engines that each created their own stream (a bench process builds seven, one after
    the other) sooner or later got one that shares its hardware queue with the main stream -- the two-stream overlap was gone and a
    4.7 ms Path B step took 5.3 (found as a leg that was slower inside the default bench line than alone)."""
    import threading
    key = (torch.device(device).index or 0, threading.get_ident(), int(priority))
    st = _side_streams.get(key)
    if st is None:
        mask = side_stream_cu_mask(device)
        if mask is None:
            st = torch.cuda.Stream(device=device, priority=int(priority))
        else:
            # a stream that leaves some CUs to the main chain (sar_stream_create_cu_mask), wrapped for torch's stream API
            words = (C.c_uint32 * len(mask))(*mask)
            h = C.c_void_p()
            with torch.cuda.device(device):
                check(L.load().sar_stream_create_cu_mask(words, len(mask), C.byref(h)), "sar_stream_create_cu_mask")
            st = torch.cuda.ExternalStream(h.value, device=device)
        _side_streams[key] = st
    return st


def shared_aux_stream(device, tag="aux"):
    """ONE further stream per (device, host thread, tag) for the branch launches an engine forks off its main chain (the resnet's
    down-sampling branch and weight images: "aux"; the radar front-end of a resident batch: "front"; SAR_PATHB_DS_STREAM): shared for
    the reason shared_side_stream gives"""
    import threading
    key = (torch.device(device).index or 0, threading.get_ident(), tag)
    st = _side_streams.get(key)
    if st is None:
        st = _side_streams[key] = torch.cuda.Stream(device=device)
    return st


def side_stream_cu_mask(device):
    """the CU mask of the weight-gradient stream as a list of 32-bit words, or None = every CU.  SAR_SIDE_CU_MASK:
    'off' | 'skip:<n>' (every n-th CU left to the main chain) | 'first:<k>' / 'last:<k>' (k contiguous CUs left out) | hex words"""
    spec = os.environ.get("SAR_SIDE_CU_MASK", SIDE_CU_MASK_DEFAULT)
    if not spec or spec == "off":
        return None
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    nw = (ncu + 31) // 32
    bits = [1] * ncu
    kind, _, arg = spec.partition(":")
    if kind == "skip":
        n = int(arg)
        for i in range(ncu):
            if i % n == n - 1:
                bits[i] = 0
    elif kind == "first":
        for i in range(int(arg)):
            bits[i] = 0
    elif kind == "last":
        for i in range(int(arg)):
            bits[ncu - 1 - i] = 0
    else:
        return [int(w, 16) for w in spec.split(",")]
    words = [0] * nw
    for i, b in enumerate(bits):
        if b:
            words[i // 32] |= 1 << (i % 32)
    return words


def amax(x, cell):
    """cell (1-element int32 view, zeroed by the caller) = max(cell, bits of max |x|) -- sar_amax_f32, no host sync"""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1      # rows may be strided (ld >= n)
    check(L.load().sar_amax_f32(ptr(x), x.shape[0], x.shape[1], x.stride(0), ptr(cell), stream_ptr()), "sar_amax_f32")


def bn_bound(gamma, beta, count, cell):
    """Samuelson bound of a train-mode BatchNorm output (sar_bn_bound_f32)"""
    check(L.load().sar_bn_bound_f32(ptr(_f32(gamma)), ptr(_f32(beta)), gamma.numel(), float(count), ptr(cell), stream_ptr()),
          "sar_bn_bound_f32")


def affine_bound(scale, shift, src_cell, cell):
    check(L.load().sar_affine_bound_f32(ptr(_f32(scale)), ptr(_f32(shift)), scale.numel(), ptr(src_cell), ptr(cell), stream_ptr()),
          "sar_affine_bound_f32")


# the arithmetic a conv_gemm / conv_wgrad call WITHOUT an explicit `split` argument takes (None = the fp32 kernels): the kernel
# parity suites run once per value (tests/conftest.py)
DEFAULT_SPLIT = None


TAP1_SPLIT = os.environ.get("SAR_TAP1_SPLIT", "1") == "1"      # the 1-tap temporal operator on conv_tap1_split_kernel (A/B switch)


def split_applicable(mode, V, Kc, M, taps, stride, tables=None, pro=None, transposed=False, pad=0):
    """shapes csrc/conv_gemm_split.hip is built for (the others stay on the fp32 kernels)"""
    if mode == L.SAR_CONV_GRAPH:       # read-gather graph kernel: few non-trivial gather lists, no folded prologue, 16-channel stages
        return (taps == 3 and V == 25 and 16 <= Kc <= 256 and Kc % 16 == 0 and M % 8 == 0 and pro is None and tables is not None
                and bool(tables.g_flags & L.SAR_GRAPH_FEW_DENSE) and tables.n_dense_lists <= 16)
    if mode == L.SAR_CONV_TEMPORAL and taps == 1:      # 1x1 (residual) convolution, forward form: conv_tap1_split_kernel (bf16x6 / f16x3a)
        return (TAP1_SPLIT and V == 25 and Kc >= 16 and M % 8 == 0 and stride in (1, 2) and pad == 0 and pro is None
                and not transposed)
    return mode == L.SAR_CONV_TEMPORAL and taps == 9 and V == 25 and 8 <= Kc <= 256 and M % 8 == 0 and stride in (1, 2)


def _pack_split_single(W, w_stride_tap, w_stride_c, taps, Kc, M, arith, src_off=0):
    """one tensor, packed on the spot (kernel tests / probes; the engines keep a PackedSplitWeights): (image, w_bound)"""
    pk = PackedSplitWeights(arith)
    pk.add("w", src_off, w_stride_tap, w_stride_c, 1, taps, Kc, M)
    pk.finalize(W.device)
    pk.refresh(W)
    return pk.image("w"), pk.bound("w")


def _src_bound_single(src, pro):
    """the bound of pro(src) for a stand-alone call: amax of the tensor, through the folded affine when there is one"""
    cells = torch.zeros(2, dtype=torch.int32, device=src.device)
    amax(src, cells[0:1])
    if pro is None:
        return cells[0:1]
    affine_bound(pro[0], pro[1], cells[0:1], cells[1:2])
    return cells[1:2]


def conv_gemm_route(split, bf16, mode, V, Kc, M, taps, stride, tables=None, pro=None, transposed=False, pad=0, epi=L.SAR_EPI_NONE):
    """the kernel of a conv_gemm call: a split arithmetic (sar_conv_gemm_split), "bf16" (sar_conv_gemm_bf16) or None (sar_conv_gemm_f32).
    `split` ("default" = DEFAULT_SPLIT) is kept on the shapes of split_applicable() -- the gated epilogue on the graph kernel only, the
    graph and 1-tap kernels in bf16x6 / f16x3a only -- and wins over bf16.  No library, no tensor (tables: g_flags, n_dense_lists)."""
    if split == "default":
        split = DEFAULT_SPLIT
    if (split and split_applicable(mode, V, Kc, M, taps, stride, tables, pro, transposed, pad)
            and (epi != L.SAR_EPI_ADD_GATE or mode == L.SAR_CONV_GRAPH)
            and (split in ("bf16x6", "f16x3a") or not (mode == L.SAR_CONV_GRAPH or taps == 1))):
        return split
    return "bf16" if (bf16 and M % 8 == 0 and Kc >= 16) else None


# ---- what the launch wrappers below (and the CN8 pair of sar_amd/ops8.py) share: DESIGN.md, "The convolution launch layer"
_CN = (lambda t: (ptr(_f32(t)), t.stride(0)), _f32)      # an fp32 CN operand -> (pointer, leading dimension); a per-channel vector
_REDUCING = (L.SAR_EPI_STATS, L.SAR_EPI_MASK, L.SAR_EPI_ADD_GATE)


def _fold_and_gather(d, vec, pro, tables, g_flags):
    """the folded prologue's affine and the gather tables of a ConvDesc / WgradDesc"""
    if pro is not None:
        d.pro_scale, d.pro_shift = ptr(vec(pro[0])), ptr(vec(pro[1]))
    if tables is not None:
        d.g_idx, d.g_wt, d.g_colsum = ptr(tables.idx), ptr(tables.wt), ptr(tables.colsum)
        for i in range(3):
            d.nz[i] = tables.nz[i]
        d.g_flags = g_flags


def _conv_desc(fmt, mode, src, out, B, V, T_src, T_out, Kc, M, taps, stride=1, pad=0, transposed=False, epi=L.SAR_EPI_NONE, pro=None,
               pro_relu=False, tables=None, g_flags=0, bias=None, aux=None, aux_affine=None, aux_mean=None):
    """the ConvDesc of a launch, but for its weights, second auxiliary and partials.  fmt = (operand, vec) reads the storage format:
    operand(t) -> (checked pointer, leading dimension), vec(t) -> a checked per-channel fp32 vector; src / out None: geometry only"""
    operand, vec = fmt
    d = ConvDesc()
    d.mode, d.transposed, d.B, d.V = mode, int(transposed), B, V
    d.T_src, d.T_out, d.Kc, d.M = T_src, T_out, Kc, M
    d.taps, d.stride, d.pad, d.pro_relu, d.epi = taps, stride, pad, int(pro_relu), epi
    if src is not None:
        d.src, d.ld_src = operand(src)
        d.out, d.ld_out = operand(out)
    d.bias = ptr(vec(bias))
    _fold_and_gather(d, vec, pro, tables, g_flags)
    if aux is not None:
        d.aux, d.ld_aux = operand(aux)
    if aux_affine is not None:
        d.aux_scale, d.aux_shift = ptr(vec(aux_affine[0])), ptr(vec(aux_affine[1]))
    d.aux_mean = ptr(vec(aux_mean))
    return d


def _wgrad_desc(fmt, mode, src, dout, B, V, T_src, T_out, Kc, M, taps, stride, pad, pro, pro_relu, tables, g_flags,
                w_stride_tap, w_stride_c, wsize, bsize):
    """the WgradDesc of a launch, but for nsplit and the slab; fmt as in _conv_desc"""
    operand, vec = fmt
    d = WgradDesc()
    d.mode, d.B, d.V, d.T_src, d.T_out, d.Kc, d.M = mode, B, V, T_src, T_out, Kc, M
    d.taps, d.stride, d.pad, d.pro_relu = taps, stride, pad, int(pro_relu)
    d.src, d.ld_src = operand(src)
    d.dout, d.ld_dout = operand(dout)
    _fold_and_gather(d, vec, pro, tables, g_flags)
    d.w_stride_tap, d.w_stride_c, d.wsize, d.bsize = w_stride_tap, w_stride_c, wsize, bsize
    return d


def _reducing_partials(d, nparts, what, M, device, partials_out=None):
    """d.partials = the (M, nparts, 2) partial sums of a reducing epilogue, returned.  nparts: the answer of the route's `nparts` query,
    raised under the name `what` when it is no count; partials_out: caller-owned rows of a stacked partials tensor (sar_amd/stgin.py)"""
    if nparts <= 0:
        check(nparts or -1, what)
    if partials_out is None:
        partials_out = torch.empty((M, nparts, 2), dtype=torch.float32, device=device)
    assert partials_out.shape == (M, nparts, 2) and partials_out.is_contiguous()
    d.partials = ptr(partials_out)
    return partials_out


def _wgrad_slab(d, slabs, out, nsplit, n, device):
    """d.nsplit, d.slab and the (nsplit, n) slab of the weight gradient that ends in out[0:n]: the batch's (a SlabBatch) or its own"""
    assert out.numel() >= n and out.is_contiguous()
    slab = slabs.slab(out, nsplit, n) if slabs is not None else torch.empty((nsplit, n), dtype=torch.float32, device=device)
    d.nsplit, d.slab = nsplit, ptr(slab)
    return slab


def _wgrad_slab_done(slabs, slab, nsplit, n, out):
    """behind the weight-gradient launch: the slabs are summed by the batch's next flush(), or by a launch of their own"""
    if slabs is not None:
        return slabs.add(slab, nsplit, n, out)
    check(L.load().sar_slab_reduce_f32(ptr(slab), nsplit, n, n, ptr(out), stream_ptr()), "sar_slab_reduce_f32")


def _split_inputs(split, bounds, sources, packed=None, pack=None):
    """([bound cell, bound cell], operand image) of a split launch.  The engines hand in all of it (sar_amd/split_plan.py); a stand-alone
    call (kernel tests, probes) leaves None what device kernels make here: first the image and the second cell = its weight bound by
    pack() -> (image, w_bound), then, for the fp16 arithmetics, the missing cell of every (tensor, folded affine) of `sources`"""
    cells = list(bounds) if bounds is not None else [None, None]
    if pack is not None and packed is None:
        packed, cells[1] = pack()
    if split.startswith("f16"):
        for i, (t, pro) in enumerate(sources):
            if cells[i] is None:
                cells[i] = _src_bound_single(t, pro)
    return cells, packed


def conv_gemm(mode, src, out, W, w_stride_tap, w_stride_c, *, B, V, T_src, T_out, Kc, M, taps, stride=1, pad=0,
              transposed=False, bias=None, pro=None, pro_relu=False, tables=None, epi=L.SAR_EPI_NONE, aux=None,
              aux_affine=None, aux_mean=None, bf16=False, packed=None, partials_out=None, aux2=None, aux_mask=None,
              split="default", bounds=None, aux_even_frames=False):
    """Launch sar_conv_gemm_f32 -- or, with bf16=True, sar_conv_gemm_bf16 (M % 8 == 0, Kc >= 16: bf16 MFMA operands, fp32 everything
    else; other shapes stay on the fp32 kernel); or, with split="bf16x6", the fp32-accurate split arithmetic on the bf16 / fp16 matrix
    pipe (sar_conv_gemm_split; `packed` = the PackedSplitWeights image or None = pack here; bounds = (src_bound, w_bound) cells for the
    fp16 arithmetics, None = computed here by device kernels).  Returns (partials, nparts) when the epilogue reduces, else None."""
    lib = L.load()
    route = conv_gemm_route(split, bf16, mode, V, Kc, M, taps, stride, tables, pro, transposed, pad, epi)
    bf16 = route == "bf16"
    split = None if bf16 else route
    # aux_even_frames: `aux` holds the even output frames only (include/sar_hip.h SAR_GRAPH_AUX_EVEN_FRAMES: the skip gradient through a
    # stride-2 residual convolution, computed compactly)
    g_flags = 0 if tables is None else (tables.g_flags | (L.SAR_GRAPH_ONE_TILE_WG if GRAPH_ONE_TILE_WG else 0)
                                        | (L.SAR_GRAPH_AUX_EVEN_FRAMES if aux_even_frames else 0))
    d = _conv_desc(_CN, mode, src, out, B, V, T_src, T_out, Kc, M, taps, stride, pad, transposed, epi, pro, pro_relu, tables, g_flags,
                   bias, aux, aux_affine, aux_mean)
    _f32(W)
    use_packed = split or (bf16 and packed is not None)      # packed: the operand image from PackedWeights (W is then not read)
    d.W, d.w_stride_tap, d.w_stride_c = (None if use_packed else ptr(W)), w_stride_tap, w_stride_c
    if epi == L.SAR_EPI_ADD_GATE:      # fp32 kernel only: aux2 [M][ld] floats, aux_mask [M][ld / 4] bytes (relu_mask layout)
        assert not bf16 and aux2 is not None and aux_mask is not None and aux_mask.dtype == torch.uint8
        assert aux2.stride(0) % 4 == 0 and aux_mask.shape == (M, aux2.stride(0) // 4) and aux_mask.is_contiguous()
        d.aux2, d.ld_aux2, d.aux_mask = ptr(_f32(aux2)), aux2.stride(0), ptr(aux_mask)
    partials, nparts = None, 0
    if epi in _REDUCING:
        nparts = lib.sar_conv_gemm_split_nparts(C.byref(d)) if split else lib.sar_conv_gemm_nparts(C.byref(d))
        partials = _reducing_partials(d, nparts, "sar_conv_gemm_nparts", M, src.device, partials_out)
    # algorithmic work: the forward conv's MACs (a data gradient costs the same MACs as its forward conv)
    n_conv = B * (T_src if transposed else T_out) * V
    flops, nbytes = 2.0 * M * Kc * taps * n_conv, 4.0 * (Kc * B * T_src * V + M * B * T_out * V)
    tag = ("gemm_graph" if mode == L.SAR_CONV_GRAPH else ("gemm_temporal%d%s" % (taps, "_dgrad" if transposed else "")))
    if split:
        (src_bound, w_bound), packed = _split_inputs(split, bounds, ((src, pro),), packed,
                                                     lambda: _pack_split_single(W, w_stride_tap, w_stride_c, taps, Kc, M, split))
        with profiler.region(tag + "_split", flops, nbytes):
            check(lib.sar_conv_gemm_split(C.byref(d), L.SAR_SPLIT[split], ptr(packed), ptr(src_bound), ptr(w_bound), stream_ptr()),
                  "sar_conv_gemm_split")
    elif bf16:
        ws = packed if use_packed else torch.empty(lib.sar_conv_gemm_bf16_workspace_bytes(C.byref(d)), dtype=torch.uint8,
                                                   device=src.device)
        with profiler.region(tag + "_bf16", flops, nbytes):
            check(lib.sar_conv_gemm_bf16(C.byref(d), ptr(ws), stream_ptr()), "sar_conv_gemm_bf16")
    else:
        with profiler.region(tag, flops, nbytes):
            check(lib.sar_conv_gemm_f32(C.byref(d), stream_ptr()), "sar_conv_gemm_f32")
    return (partials, nparts) if partials is not None else None


def conv_gemm_nparts(B, V, T_src, T_out, Kc, M, taps=1, stride=1, pad=0, transposed=False, epi=L.SAR_EPI_STATS):
    """partial sums per output row that sar_conv_gemm_f32 (TEMPORAL) writes for this geometry"""
    d = _conv_desc(_CN, L.SAR_CONV_TEMPORAL, None, None, B, V, T_src, T_out, Kc, M, taps, stride, pad, transposed, epi)
    n = L.load().sar_conv_gemm_nparts(C.byref(d))
    if n <= 0:
        check(n or -1, "sar_conv_gemm_nparts")
    return n


_WGRAD1_SLOTS = int(os.environ.get("SAR_WGRAD1_SLOTS", "1024"))      # workgroups in flight of the 1-tap weight gradients
_WGRAD9_SLOTS = int(os.environ.get("SAR_WGRAD9_SLOTS", "1024"))      # ... of the 9-tap temporal ones (sweep knobs)
_WGRADG_SLOTS = int(os.environ.get("SAR_WGRADG_SLOTS", "512"))       # ... of the graph ones

# columns per workgroup of the first layer's streaming weight gradient (graph_wgrad_small4_kernel: 256-column iterations)
_WGRAD_SMALL_COLS = int(os.environ.get("SAR_WGRAD_SMALL_COLS", "4096"))

# SAR_SLAB_BATCH=0: every weight gradient reduces its slabs by its own launch again (A/B switch)
SLAB_BATCH = os.environ.get("SAR_SLAB_BATCH", "1") == "1"
# when an engine flushes its batch: "end" = at the end of backward (and before a bucket goes to the all-reduce), "bucket" = at every
# bucket boundary also without a data-parallel callback, "block" = behind every block
SLAB_FLUSH = os.environ.get("SAR_SLAB_FLUSH", "end")


class SlabBatch:
    """The partial slabs of the weight gradients of a backward pass, summed by ONE launch per flush() (sar_slab_reduce_batch_f32:
    per element the additions of sar_slab_reduce_f32 in the same order -- bit-identical) instead of one launch behind every
    weight-gradient kernel: a step had 20-22 of them, 3-4 % of the fp32-storage steps (tools/skip_probe.py).  The slab buffers are
    owned here and re-used every step (key = the destination slice of the flat gradient buffer), so a flush of the same items finds
    its device table in the cache.  Everything -- weight-gradient kernels and flush() -- must be issued on ONE stream (the engines'
    weight-gradient stream); an engine flushes before a gradient bucket is handed to the all-reduce and at the end of backward."""

    ITEM = [("slab", "<u8"), ("out", "<u8"), ("stride", "<i8"), ("n", "<i8"), ("nsplit", "<i4"), ("reserved", "<i4")]

    def __init__(self):
        self._slabs, self._pending, self._tables = {}, [], {}

    def slab(self, out, nsplit, n):
        """the (nsplit, n) slab buffer of the weight gradient that ends in out[0:n]"""
        key = (out.data_ptr(), nsplit, n)
        t = self._slabs.get(key)
        if t is None:
            if len(self._slabs) >= 512:      # a caller that keeps changing its batch geometry: do not grow without bound
                assert not self._pending, "SlabBatch: slab buffers would be dropped with reductions pending"
                self._slabs.clear()
                self._tables.clear()
            t = self._slabs[key] = torch.empty((nsplit, n), dtype=torch.float32, device=out.device)
        return t

    def add(self, slab, nsplit, n, out):
        assert out.numel() >= n and out.is_contiguous() and slab.stride(0) >= n
        self._pending.append((slab.data_ptr(), out.data_ptr(), slab.stride(0), n, nsplit, 0))
        self._device = slab.device

    def flush(self):
        if not self._pending:
            return
        key, self._pending = tuple(self._pending), []
        ent = self._tables.get(key)
        if ent is None:
            import numpy as np
            tab = np.array(list(key), dtype=np.dtype(self.ITEM, align=True))
            assert tab.dtype.itemsize == 40          # sizeof(sar_slab_item)
            ent = self._tables[key] = (torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(self._device), max(it[3] for it in key))
        check(L.load().sar_slab_reduce_batch_f32(ptr(ent[0]), len(key), ent[1], stream_ptr()), "sar_slab_reduce_batch_f32")


def conv_wgrad_route(split, bf16, mode, V, taps, stride, pad, blocks):
    """(kernel, sp) of a conv_wgrad call: a split arithmetic (sar_conv_wgrad_split: bf16x6 / f16x3a where blocks(arith) -> sp =
    (workgroups, wk, kt), the answer of sar_conv_wgrad_split_blocks for the call's geometry, counts workgroups), "bf16"
    (sar_conv_wgrad_bf16) or None (sar_conv_wgrad_f32).  `split`: "default" = DEFAULT_SPLIT."""
    if split == "default":
        split = DEFAULT_SPLIT
    if split in ("bf16x6", "f16x3a") and not (taps == 1 and mode == L.SAR_CONV_TEMPORAL and not TAP1_SPLIT):
        sp = blocks(split)
        if sp[0] > 0:
            return split, sp
    # (a bf16 graph weight gradient was built and measured: with the adjacency gather in its stager it ran 1.7x SLOWER
    # than the fp32 kernel -- 9.0 vs 5.4 ms per step -- so the graph weight gradient stays on the fp32 kernel)
    if bf16 and mode == L.SAR_CONV_TEMPORAL and taps == 9 and V == 25 and (stride == 1 or (stride == 2 and pad == 3)):
        return "bf16", None
    return None, None


def conv_wgrad_nsplit(route, sp, nsplit, mode, B, V, T_out, Kc, M, taps, stride, pro=None):
    """the slabs of a conv_wgrad launch: the caller's `nsplit` (rounded up to the split kernel's multiple) or the default of the kernel
    that runs; (route, sp) as conv_wgrad_route returns them"""
    if route not in (None, "bf16"):
        sp_blocks, wk, kt = sp
        if nsplit is None:      # one round of the 512 resident workgroups (two per CU); SAR_WGRAD_SPLIT_SLOTS: experiment
            ntiles = B * ((T_out * V + kt - 1) // kt)
            return max(1, min(ntiles, _WGRADS_SLOTS // sp_blocks)) * wk
        return (nsplit + wk - 1) // wk * wk
    if nsplit is not None:
        return nsplit
    if route == "bf16":     # 64 (m) x 64 / 32 (c, stride 1 / 2) weight blocks, 8-frame tiles; one round of the 512 resident workgroups
        ntiles = B * ((T_out + 7) // 8)
        cb = 64 if stride == 1 else 32
        return max(1, min(ntiles, 512 // (((M + 63) // 64) * ((Kc + cb - 1) // cb))))
    if mode == L.SAR_CONV_GRAPH and Kc <= 4 and pro is None:
        # streaming kernel of the 3-channel first layer (conv_wgrad.hip: graph_wgrad_small_kernel): ~8 chunks of 64 columns per
        # workgroup (its loop is latency-bound: many short workgroups, not few long ones)
        return max(1, min(4096, (B * T_out * V + _WGRAD_SMALL_COLS - 1) // _WGRAD_SMALL_COLS))
    ct = 32 if (mode == L.SAR_CONV_TEMPORAL and taps == 9) else 64
    ft, bf = max(2, min((128 // V) & ~1, (T_out + 1) & ~1)), 64
    if mode == L.SAR_CONV_GRAPH and V == 25 and Kc >= 32 and pro is None:      # fixed-geometry kernel: 2-frame tiles, 128 x 64 blocks when M > 64
        ft, bf = 2, (128 if M > 64 else 64)
    ntiles = B * ((T_out + ft - 1) // ft)
    wgs = ((M + bf - 1) // bf) * ((Kc + ct - 1) // ct)
    # workgroups in flight: two rounds of the 512 resident slots for the temporal kernels, one for the graph kernel
    # (tools/nsplit_sweep.py)
    target = _WGRADG_SLOTS if (mode == L.SAR_CONV_GRAPH and ft == 2) else (_WGRAD1_SLOTS if taps == 1 else _WGRAD9_SLOTS)
    return max(1, min(ntiles, (target + wgs - 1) // wgs))


def conv_wgrad(mode, src, dout, dW_out, *, B, V, T_src, T_out, Kc, M, taps, stride=1, pad=0, pro=None, pro_relu=False,
               tables=None, w_stride_tap, w_stride_c, wsize, bsize, nsplit=None, bf16=False, split="default", bounds=None,
               slabs=None):
    """dW (and dbias, stored right behind it) -> dW_out[0 : wsize+bsize] (flat float32 view).  bf16=True routes the
    9-tap temporal operator (V = 25; stride 1, or stride 2 with the even-T SAME padding 3) to sar_conv_wgrad_bf16 (bf16 MFMA operands, fp32 accumulation and bias
    sums); every other shape stays on the fp32 kernel.  split="bf16x6" / "f16x3a": the split arithmetic of csrc/conv_wgrad_split.hip
    where it is built (bounds = (src_bound, dout_bound) cells for the fp16 arithmetic, None = computed here by device kernels); other
    shapes stay on the fp32 kernel.  slabs (SlabBatch): the slabs are summed by the batch's next flush() instead of by a launch of
    their own."""
    lib = L.load()
    d = _wgrad_desc(_CN, mode, src, dout, B, V, T_src, T_out, Kc, M, taps, stride, pad, pro, pro_relu, tables,
                    tables.g_flags if tables is not None else 0, w_stride_tap, w_stride_c, wsize, bsize)
    def blocks(arith):      # (what the route asks the library)
        wk, kt = C.c_int(0), C.c_int(0)
        return lib.sar_conv_wgrad_split_blocks(C.byref(d), L.SAR_SPLIT[arith], C.byref(wk), C.byref(kt)), wk.value, kt.value
    route, sp = conv_wgrad_route(split, bf16, mode, V, taps, stride, pad, blocks)
    nsplit, n = conv_wgrad_nsplit(route, sp, nsplit, mode, B, V, T_out, Kc, M, taps, stride, pro), wsize + bsize
    slab = _wgrad_slab(d, slabs, dW_out, nsplit, n, src.device)
    tag = "wgrad_graph" if mode == L.SAR_CONV_GRAPH else "wgrad_temporal%d" % taps
    flops, nbytes = 2.0 * M * Kc * taps * B * T_out * V, 4.0 * (Kc * B * T_src * V + M * B * T_out * V)
    split = route if route != "bf16" else None
    if split:      # (cells handed in are taken as they are; with none, both are made here)
        (src_bound, dout_bound), _ = _split_inputs(split, bounds, ((src, pro), (dout, None)) if bounds is None else ())
    with profiler.region(tag + ("_split" if split else "_bf16" if route else ""), flops, nbytes):
        if split:
            check(lib.sar_conv_wgrad_split(C.byref(d), L.SAR_SPLIT[split], ptr(src_bound), ptr(dout_bound), stream_ptr()),
                  "sar_conv_wgrad_split")
        elif route:
            check(lib.sar_conv_wgrad_bf16(C.byref(d), stream_ptr()), "sar_conv_wgrad_bf16")
        else:
            check(lib.sar_conv_wgrad_f32(C.byref(d), stream_ptr()), "sar_conv_wgrad_f32")
    _wgrad_slab_done(slabs, slab, nsplit, n, dW_out)


# ---- the 1x1 product of every layer (models/ and the layer wrappers below): columns (B, T, V) of a CN matrix, V <= 64
# (sar_conv_gemm_f32's limit); fp32 whatever SAR_* split arithmetic is set (split=None).  `out` = rows of a caller's stacked matrix;
# **kw goes to the kernel as it is
def conv1x1_fwd(X, W, bias, geo, out=None, **kw):
    """out (M, n) = W^T X + bias; kw: pro, pro_relu (BN + ReLU on the operand load), epi, partials_out (the statistics epilogue)"""
    Kc, M = W.shape
    if out is None:
        out = torch.empty((M, X.shape[1]), dtype=torch.float32, device=X.device)
    conv_gemm(L.SAR_CONV_TEMPORAL, X, out, W, 0, M, Kc=Kc, M=M, taps=1, stride=1, pad=0, bias=bias, split=None, **geo, **kw)
    return out


def conv1x1_wgrad(X, dy, geo, **kw):
    """(dW (C M), dbias (M)) of X (C, n) and dy (M, n), one launch; kw: pro, pro_relu"""
    Kc, M = X.shape[0], dy.shape[0]
    flat = torch.empty(Kc * M + M, dtype=torch.float32, device=X.device)
    conv_wgrad(L.SAR_CONV_TEMPORAL, X, dy, flat, Kc=Kc, M=M, taps=1, stride=1, pad=0, w_stride_tap=0, w_stride_c=M, wsize=Kc * M,
               bsize=M, split=None, **geo, **kw)
    return flat[:Kc * M], flat[Kc * M:]


def conv1x1_dgrad(dy, W, geo, out=None, **kw):
    """out (C, n) = W dy; kw: epi, aux, aux_affine, aux_mean, partials_out (the masked gradient through a folded BN + ReLU)"""
    Kc, M = W.shape
    WT = torch.empty((M, Kc), dtype=torch.float32, device=dy.device)
    transpose(W, WT, 1, Kc, M)
    if out is None:
        out = torch.empty((Kc, dy.shape[1]), dtype=torch.float32, device=dy.device)
    conv_gemm(L.SAR_CONV_TEMPORAL, dy, out, WT, 0, Kc, Kc=M, M=Kc, taps=1, stride=1, pad=0, transposed=True, split=None, **geo, **kw)
    return out


def column_geometry(N, V):
    """a (B, T, V') factorisation of the N * V columns with V' <= 64: the 1x1 product does not care which"""
    vf = max(d for d in range(1, min(V, 64) + 1) if V % d == 0)
    return dict(B=N, V=vf, T_src=V // vf, T_out=V // vf)


def bn_finalize(partials, nparts, C_, count, eps, momentum, unbiased_running, gamma, beta, running_mean, running_var,
                mean, rstd, scale, shift, pivot=None):
    """pivot: the per-channel float32 value the producer subtracted before it summed (data_bn_stats), or None"""
    if pivot is not None:
        check(L.load().sar_bn_finalize_pivot_f32(ptr(partials), nparts, C_, float(count), ptr(pivot), eps, momentum,
                                                 int(unbiased_running), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                                                 ptr(mean), ptr(rstd), ptr(scale), ptr(shift), stream_ptr()),
              "sar_bn_finalize_pivot_f32")
        return
    check(L.load().sar_bn_finalize_f32(ptr(partials), nparts, C_, float(count), eps, momentum, int(unbiased_running),
                                       ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(mean), ptr(rstd),
                                       ptr(scale), ptr(shift), stream_ptr()), "sar_bn_finalize_f32")


def bn_eval_affine(gamma, beta, running_mean, running_var, eps, scale, shift):
    check(L.load().sar_bn_eval_affine_f32(ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), eps,
                                          running_mean.numel(), ptr(scale), ptr(shift), stream_ptr()),
          "sar_bn_eval_affine_f32")


def bn_bwd_finalize(partials, nparts, chan_stride, part_stride, off1, off2, C_, count, gamma, mean, rstd, dgamma, dbeta,
                    k1=None, k2=None, k3=None, centered=True):
    check(L.load().sar_bn_bwd_finalize_f32(ptr(partials), nparts, chan_stride, part_stride, off1, off2, int(centered), C_,
                                           float(count),
                                           ptr(gamma), ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta), ptr(k1), ptr(k2),
                                           ptr(k3), stream_ptr()), "sar_bn_bwd_finalize_f32")


def data_bn_stats(x, bone_parent, partials, motion=False, pivot=None):
    """partials [V*C][N][2] of the clip's BatchNorm channels.  pivot (float32 [V*C], written here): two passes, the second sums
    (x - pivot) with pivot = the first pass's mean for every channel more than 2 standard deviations from 0 (the others keep
    pivot 0 and their first-pass sums, bit for bit), for bn_finalize(.., pivot=pivot) -- what the engines run, since raw
    coordinates are not centred ("BatchNorm statistics on un-centred data").  pivot None: one pass, the sums of x, x^2."""
    N, C_, T, V, M = x.shape
    if pivot is not None:
        assert pivot.numel() == V * C_ and pivot.dtype == torch.float32 and pivot.is_contiguous()
        check(L.load().sar_data_bn_stats_pivot_f32(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(pivot), ptr(partials),
                                                   stream_ptr()), "sar_data_bn_stats_pivot_f32")
        return
    check(L.load().sar_data_bn_stats_f32(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(partials), stream_ptr()),
          "sar_data_bn_stats_f32")


def data_bn_apply(x, bone_parent, scale, shift, out, motion=False):
    N, C_, T, V, M = x.shape
    check(L.load().sar_data_bn_apply_f32(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(scale), ptr(shift), ptr(out),
                                         out.stride(0), stream_ptr()), "sar_data_bn_apply_f32")


def data_bn_bwd_reduce(x, bone_parent, dy, mean, partials, motion=False):
    N, C_, T, V, M = x.shape
    check(L.load().sar_data_bn_bwd_reduce_f32(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(dy), dy.stride(0), ptr(mean),
                                              ptr(partials), stream_ptr()), "sar_data_bn_bwd_reduce_f32")


DATA_BN_DX_FRAMES = 16    # frames of dx per workgroup of data_bn_bwd_apply (= sar_data_bn_dx_frames(); tests/test_data_bn_dx_abi.py)


def _data_bn_dx_out(x, dx):
    """the (N, C, T, V, M) float32 output of the backward apply pass"""
    assert x.dim() == 5 and x.dtype == torch.float32 and x.is_cuda and x.is_contiguous(), "need a contiguous cuda float32 clip"
    if dx is None:
        dx = torch.empty_like(x)
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_cuda and dx.is_contiguous()
    return dx


def data_bn_bwd_apply(x, bone_parent, dy, k, dx=None, motion=False):
    """d loss / d x (N, C, T, V, M) from dy = d loss / d data_bn(x) (CN rows [C][ld >= N*M*T*V]) and k = (k1, k2, k3) of
    bn_bwd_finalize; include/sar_hip.h has the formulas"""
    dx = _data_bn_dx_out(x, dx)
    N, C_, T, V, M = x.shape
    assert _f32(dy).dim() == 2 and dy.shape[0] == C_
    ld = dy.stride(0) if C_ > 1 else dy.shape[1]        # (torch gives a single row whatever stride it likes: its width counts)
    check(L.load().sar_data_bn_bwd_apply_f32(ptr(x), N, C_, T, V, M, ptr(bone_parent), int(motion), ptr(dy), ld,
                                             ptr(_f32(k[0])), ptr(_f32(k[1])), ptr(_f32(k[2])), ptr(dx), stream_ptr()),
          "sar_data_bn_bwd_apply_f32")
    return dx


RELU_MASK = os.environ.get("SAR_RELU_MASK", "1") == "1"   # block tails write / read a 1-bit ReLU mask (A/B switch)


def relu_mask(u):
    """the mask tensor of a (C, n) fp32 block-tail output: one byte per float4, or None when the rows are not 4-element groups"""
    Cc, n = u.shape
    if not RELU_MASK or n % 4 or u.stride(0) % 4:
        return None
    return torch.empty((Cc, u.stride(0) // 4), dtype=torch.uint8, device=u.device)


def bn_add_relu_fwd(u, sc, sh, res_kind, r, rsc, rsh, y, mask=None, amax_cell=None):
    """mask (relu_mask): written beside y.  amax_cell: the bound cell of y (split arithmetic), raised by the pass itself"""
    check(L.load().sar_bn_add_relu_fwd_f32(ptr(u), ptr(sc), ptr(sh), res_kind, ptr(r), ptr(rsc), ptr(rsh), ptr(y), ptr(mask),
                                           ptr(amax_cell), u.shape[0], u.shape[1], u.stride(0), stream_ptr()),
          "sar_bn_add_relu_fwd_f32")


_REDUCE_CHUNK = int(os.environ.get("SAR_BWD_REDUCE_CHUNK", "8192"))      # row elements per workgroup of the BN-backward reductions


# SAR_BN_TAIL=1: the BatchNorm-backward finalisation of every block tail runs in the reduce kernel's last workgroup instead of in
# its own launch(es).  Measured (three interleaved rounds each): fp32 59.44 vs 59.49 ms, bf16 13.37 vs 13.32, Path B 6.35 vs 6.37
# -- the launches it removes were waiting beside useful work of the other stream, not in front of it.  OFF by default: the sc1
# hand-off it relies on is measured behaviour of this part (MI355X_MICROARCH.md), not an architectural guarantee, and buys nothing.
BN_TAIL = os.environ.get("SAR_BN_TAIL", "0") == "1"
_tickets = {}


def bn_tail_tickets(device):
    """the ticket array of the folded finalisations, one per (device, stream): launches on ONE stream run one after the other and
    share it (4096 ints, zero; every launch leaves it zero); two host threads on two streams never share one"""
    key = (str(device), stream_ptr())
    if key not in _tickets:
        _tickets[key] = torch.zeros(4096, dtype=torch.int32, device=device)
    return _tickets[key]


def make_bn_tail(device, count, gamma, bn, dgamma, dbeta, rgamma=None, rbn=None, rdgamma=None, rdbeta=None):
    """sar_bn_tail for a block tail: bn / rbn are _BN records (rstd, k1, k2, k3)"""
    t = L.BnTail()
    t.ticket, t.count = ptr(bn_tail_tickets(device)), float(count)
    t.gamma, t.rstd, t.dgamma, t.dbeta = ptr(_f32(gamma)), ptr(bn.rstd), ptr(_f32(dgamma)), ptr(_f32(dbeta))
    t.k1, t.k2, t.k3 = ptr(bn.k1), ptr(bn.k2), ptr(bn.k3)
    if rbn is not None:
        t.rgamma, t.rrstd, t.rdgamma, t.rdbeta = ptr(_f32(rgamma)), ptr(rbn.rstd), ptr(_f32(rdgamma)), ptr(_f32(rdbeta))
        t.rk1, t.rk2, t.rk3 = ptr(rbn.k1), ptr(rbn.k2), ptr(rbn.k3)
    return t


def bn_add_relu_bwd_reduce(dy, y, u, r, mu=None, mr=None, tail=None, mask=None):
    """tail (make_bn_tail): the reduce kernel's last workgroup per channel also finalises (dgamma, dbeta, k1..k3): no
    sar_bn_bwd_finalize launch behind it.  mask (relu_mask, written by bn_add_relu_fwd): read instead of y."""
    Cc, n = u.shape
    nparts = max(1, min(4096, (n + _REDUCE_CHUNK - 1) // _REDUCE_CHUNK))
    partials = torch.empty((Cc, nparts, 4), dtype=torch.float32, device=u.device)
    assert tail is None or Cc <= 4096        # bn_tail_tickets
    # with a tail the pass keeps reading y, as it always has: the mask is passed only without one
    check(L.load().sar_bn_add_relu_bwd_reduce_f32(ptr(dy), ptr(y), ptr(mask if tail is None else None), ptr(u), ptr(r), ptr(mu), ptr(mr),
                                                  ptr(partials), nparts, Cc, n, u.stride(0),
                                                  C.byref(tail) if tail is not None else None, stream_ptr()),
          "sar_bn_add_relu_bwd_reduce_f32")
    return partials, nparts


def bn_add_relu_bwd_apply(dy, y, u, r, k, rk, du, dr, dz_out, mask=None, amax_cell=None, amax_dr_cell=None):
    """amax_cell: the bound cell of du (split arithmetic), see bn_add_relu_fwd; amax_dr_cell: the same for dr (the operand of the
    residual branch's dense 1x1 data gradient)"""
    Cc, n = u.shape
    rk = rk or (None, None, None)
    check(L.load().sar_bn_add_relu_bwd_apply_f32(ptr(dy), ptr(y), ptr(mask), ptr(u), ptr(r), ptr(k[0]), ptr(k[1]), ptr(k[2]),
                                                 ptr(rk[0]), ptr(rk[1]), ptr(rk[2]), ptr(du), ptr(dr), ptr(dz_out), ptr(amax_cell),
                                                 ptr(amax_dr_cell if dr is not None else None), Cc, n, u.stride(0), stream_ptr()),
          "sar_bn_add_relu_bwd_apply_f32")


def affine2(a, b, k, out, amax_cell=None):
    Cc, n = a.shape
    check(L.load().sar_affine2_f32(ptr(a), ptr(b), ptr(k[0]), ptr(k[1]), ptr(k[2]), ptr(out), ptr(amax_cell), Cc, n, a.stride(0),
                                   stream_ptr()), "sar_affine2_f32")


def pool_fwd(y, B, TV, Mp, feat):
    check(L.load().sar_pool_fwd_f32(ptr(y), y.stride(0), y.shape[0], B, TV, Mp, ptr(feat), stream_ptr()),
          "sar_pool_fwd_f32")


def fc_fwd(feat, W, bias, logits):
    N, Cc = feat.shape
    check(L.load().sar_fc_fwd_f32(ptr(feat), ptr(W), ptr(bias), N, Cc, logits.shape[1], ptr(logits), stream_ptr()),
          "sar_fc_fwd_f32")


def softmax_ce(logits, labels, inv_global_batch, loss_sum=None, dlogits=None, probs=None):
    N, K = logits.shape
    assert labels.dtype == torch.int64 and labels.is_cuda
    check(L.load().sar_softmax_ce_f32(ptr(logits), ptr(labels), N, K, inv_global_batch, ptr(loss_sum), ptr(dlogits),
                                      ptr(probs), stream_ptr()), "sar_softmax_ce_f32")


def fc_bwd(feat, W, dlogits, dW, dbias, dfeat):
    N, Cc = feat.shape
    check(L.load().sar_fc_bwd_f32(ptr(feat), ptr(W), ptr(dlogits), N, Cc, dlogits.shape[1], ptr(dW), ptr(dbias),
                                  ptr(dfeat), stream_ptr()), "sar_fc_bwd_f32")


def pool_bwd(dfeat, B, TV, Mp, dy):
    check(L.load().sar_pool_bwd_f32(ptr(dfeat), dy.stride(0), dy.shape[0], B, TV, Mp, ptr(dy), stream_ptr()),
          "sar_pool_bwd_f32")


def sgd_nesterov(w, v, g, lr_dev, momentum):
    check(L.load().sar_sgd_nesterov_f32(ptr(w), ptr(v), ptr(g), w.numel(), ptr(lr_dev), momentum, stream_ptr()),
          "sar_sgd_nesterov_f32")


def transpose(inp, out, batch, R, Cc):
    check(L.load().sar_transpose_f32(ptr(inp), ptr(out), batch, R, Cc, stream_ptr()), "sar_transpose_f32")


def pre_normalize(x, out=None, zaxis=(0, 1), xaxis=(8, 4)):
    """data_gen/preprocess.py `pre_normalization` of a batch of raw clips (N, 3, T, V, M) on the device (csrc/prenorm.hip): null
    frames padded by looping the clip, centred on body 0's joint 1, bone zaxis onto z, bone xaxis onto x.  Returns `out` (a new
    tensor when None); `out` must not overlap x."""
    _f32(x)
    if x.dim() != 5 or x.shape[1] != 3:
        raise L.SarError("pre_normalize: need (N, 3, T, V, M) coordinates, got %s" % (tuple(x.shape),))
    if out is None:
        out = torch.empty_like(x)
    _f32(out)
    if out.shape != x.shape:
        raise L.SarError("pre_normalize: out %s does not match x %s" % (tuple(out.shape), tuple(x.shape)))
    N, _, T, V, M = x.shape
    check(L.load().sar_pre_normalize_f32(ptr(x), ptr(out), N, T, V, M, int(zaxis[0]), int(zaxis[1]), int(xaxis[0]), int(xaxis[1]),
                                         stream_ptr()), "sar_pre_normalize_f32")
    return out


AUGMENT_MAX_T, AUGMENT_MAX_V, AUGMENT_MAX_M = 2048, 32, 4      # csrc/augment.hip AG_MAX_*


def augment_clips(x, params, crop=False, out=None):
    """Training-time augmentation of a batch of clips (N, 3, T, V, M) on the device (csrc/augment.hip): per clip a temporal
    crop-resize (only with `crop`), then a per-frame rotation, scale and shift between two key frames.  `params` is the (N, 16)
    float32 table of sar_amd.augment.ClipAugment.table on x's device.  Returns `out` (a new tensor when None); `out` must not
    overlap x.  Every argument error is raised before the library is touched."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise L.SarError("augment_clips: x must be a contiguous cuda float32 tensor")
    if x.dim() != 5 or x.shape[1] != 3:
        raise L.SarError("augment_clips: need (N, 3, T, V, M) coordinates, got %s" % (tuple(x.shape),))
    N, _, T, V, M = x.shape
    if not (torch.is_tensor(params) and params.dtype == torch.float32 and params.device == x.device and params.is_contiguous()
            and tuple(params.shape) == (N, 16)):
        raise L.SarError("augment_clips: params must be a contiguous (%d, 16) float32 tensor on %s" % (N, x.device))
    if T < 1 or V < 1 or M < 1 or T > AUGMENT_MAX_T or V > AUGMENT_MAX_V or M > AUGMENT_MAX_M:
        raise L.SarError("augment_clips: built for 1 <= T <= %d, V <= %d, M <= %d (got T %d V %d M %d)"
                         % (AUGMENT_MAX_T, AUGMENT_MAX_V, AUGMENT_MAX_M, T, V, M))
    if out is None:
        out = torch.empty_like(x)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device):
        raise L.SarError("augment_clips: out must be a contiguous cuda float32 tensor on x's device")
    if out.shape != x.shape:
        raise L.SarError("augment_clips: out %s does not match x %s" % (tuple(out.shape), tuple(x.shape)))
    nbytes = x.numel() * 4
    for name, other, nb in (("x", x, nbytes), ("params", params, params.numel() * 4)):
        if nbytes and nb and out.data_ptr() < other.data_ptr() + nb and other.data_ptr() < out.data_ptr() + nbytes:
            raise L.SarError("augment_clips: out must not overlap %s" % name)
    check(L.load().sar_augment_clips_f32(ptr(x), ptr(params), ptr(out), N, T, V, M, int(bool(crop)), stream_ptr()),
          "sar_augment_clips_f32")
    return out


# ------------------------------------------------------------------------------------------------ dense adjacency
def graph_dense_fwd(y, A, out, K, F, V, nframes, stats=False, add=None):
    """out[m] = sum_k y[k F + m] . A_k (+ add[m]) (sar_graph_dense_fwd_f32); returns (partials, nparts) when stats."""
    lib = L.load()
    partials, nparts = None, 0
    if stats:
        nparts = lib.sar_graph_dense_nparts(nframes)
        partials = torch.empty((F, nparts, 2), dtype=torch.float32, device=y.device)
    check(lib.sar_graph_dense_fwd_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(A)), ptr(_f32(out)), out.stride(0), K, F, V, nframes,
                                      ptr(partials), ptr(_f32(add)), add.stride(0) if add is not None else 0, stream_ptr()),
          "sar_graph_dense_fwd_f32")
    return (partials, nparts) if stats else None


def graph_dense_bwd_data(dout, A, dy, K, F, V, nframes):
    check(L.load().sar_graph_dense_bwd_data_f32(ptr(_f32(dout)), dout.stride(0), ptr(_f32(A)), ptr(_f32(dy)), dy.stride(0), K, F, V,
                                                nframes, stream_ptr()), "sar_graph_dense_bwd_data_f32")


def graph_dense_dA(y, dout, dA, K, F, V, nframes, nsplit=64):
    lib = L.load()
    nsplit = max(1, min(nsplit, (nframes + 7) // 8))
    slab = torch.empty(lib.sar_graph_dense_dadj_slab_floats(K, F, V, nsplit), dtype=torch.float32, device=y.device)
    check(lib.sar_graph_dense_dadj_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(dout)), dout.stride(0), K, F, V, nframes, nsplit,
                                     ptr(slab), ptr(_f32(dA)), stream_ptr()), "sar_graph_dense_dadj_f32")


# ------------------------------------------------------------------------------------------------ dense adjacency per frame
def graph_dense_t_fwd(y, At, out, K, F, V, B, T, stats=False, add=None):
    """out[m, (b,t,:)] = sum_k y[k F + m, (b,t,:)] . At[k, t] (+ add[m]) (sar_graph_dense_t_fwd_f32); At (K, T, V, V) contiguous;
    returns (partials, nparts) when stats."""
    lib = L.load()
    assert At.is_contiguous() and tuple(At.shape) == (K, T, V, V), "At must be a contiguous (K, T, V, V) table"
    partials, nparts = None, 0
    if stats:
        nparts = lib.sar_graph_dense_t_nparts(B, T)
        partials = torch.empty((F, nparts, 2), dtype=torch.float32, device=y.device)
    check(lib.sar_graph_dense_t_fwd_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(At)), ptr(_f32(out)), out.stride(0), K, F, V, B, T,
                                        ptr(partials), ptr(_f32(add)), add.stride(0) if add is not None else 0, stream_ptr()),
          "sar_graph_dense_t_fwd_f32")
    return (partials, nparts) if stats else None


def graph_dense_t_bwd_data(dout, At, dy, K, F, V, B, T):
    assert At.is_contiguous() and tuple(At.shape) == (K, T, V, V), "At must be a contiguous (K, T, V, V) table"
    check(L.load().sar_graph_dense_t_bwd_data_f32(ptr(_f32(dout)), dout.stride(0), ptr(_f32(At)), ptr(_f32(dy)), dy.stride(0), K, F, V,
                                                  B, T, stream_ptr()), "sar_graph_dense_t_bwd_data_f32")


def graph_dense_t_dA(y, dout, dAt, K, F, V, B, T):
    """dAt (K, T, V, V) contiguous = sum over channels and samples of y (x) dout per frame (sar_graph_dense_t_dadj_f32)"""
    lib = L.load()
    assert dAt.is_contiguous() and dAt.numel() == K * T * V * V
    slab = torch.empty(lib.sar_graph_dense_t_dadj_slab_floats(K, V, B, T), dtype=torch.float32, device=y.device)
    check(lib.sar_graph_dense_t_dadj_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(dout)), dout.stride(0), K, F, V, B, T, ptr(slab),
                                         ptr(_f32(dAt)), stream_ptr()), "sar_graph_dense_t_dadj_f32")


# ------------------------------------------------------------------------------------------------ adjacency per sample
def graph_sample_fwd(y, A, out, F, V, N):
    """out[m, (n,:)] = y[m, (n,:)] . A[n] (sar_graph_sample_fwd_f32); A (N, V, V) contiguous, y / out CN rows of >= N V columns"""
    assert A.is_contiguous() and tuple(A.shape) == (N, V, V), "A must be a contiguous (N, V, V) table"
    check(L.load().sar_graph_sample_fwd_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(A)), ptr(_f32(out)), out.stride(0), F, V, N,
                                            stream_ptr()), "sar_graph_sample_fwd_f32")


def graph_sample_bwd_data(dout, A, dy, F, V, N):
    """dy[m, (n,:)] = dout[m, (n,:)] . A[n]^T (sar_graph_sample_bwd_data_f32)"""
    assert A.is_contiguous() and tuple(A.shape) == (N, V, V), "A must be a contiguous (N, V, V) table"
    check(L.load().sar_graph_sample_bwd_data_f32(ptr(_f32(dout)), dout.stride(0), ptr(_f32(A)), ptr(_f32(dy)), dy.stride(0), F, V, N,
                                                 stream_ptr()), "sar_graph_sample_bwd_data_f32")


def graph_sample_dA(y, dout, dA, F, V, N):
    """dA (N, V, V) contiguous: dA[n] = y[:, (n,:)]^T . dout[:, (n,:)] (sar_graph_sample_dadj_f32)"""
    assert dA.is_contiguous() and tuple(dA.shape) == (N, V, V), "dA must be a contiguous (N, V, V) table"
    check(L.load().sar_graph_sample_dadj_f32(ptr(_f32(y)), y.stride(0), ptr(_f32(dout)), dout.stride(0), ptr(_f32(dA)), F, V, N,
                                             stream_ptr()), "sar_graph_sample_dadj_f32")


def gin_sample_fwd(x, A, eps, out, F, V, N):
    """out[m, (n,:)] = x[m, (n,:)] . A[n] + (1 + eps) x[m, (n,:)] (sar_gin_sample_fwd_f32); eps: the layer's scalar ON THE DEVICE"""
    assert A.is_contiguous() and tuple(A.shape) == (N, V, V), "A must be a contiguous (N, V, V) table"
    assert eps.is_cuda and eps.dtype == torch.float32 and eps.numel() == 1, "eps must be one float32 on the device"
    check(L.load().sar_gin_sample_fwd_f32(ptr(_f32(x)), x.stride(0), ptr(_f32(A)), ptr(eps), ptr(_f32(out)), out.stride(0), F, V, N,
                                          stream_ptr()), "sar_gin_sample_fwd_f32")


def gin_sample_bwd_data(dout, A, eps, dx, F, V, N):
    """dx[m, (n,:)] = dout[m, (n,:)] . A[n]^T + (1 + eps) dout[m, (n,:)] (sar_gin_sample_bwd_data_f32)"""
    assert A.is_contiguous() and tuple(A.shape) == (N, V, V), "A must be a contiguous (N, V, V) table"
    assert eps.is_cuda and eps.dtype == torch.float32 and eps.numel() == 1, "eps must be one float32 on the device"
    check(L.load().sar_gin_sample_bwd_data_f32(ptr(_f32(dout)), dout.stride(0), ptr(_f32(A)), ptr(eps), ptr(_f32(dx)), dx.stride(0),
                                               F, V, N, stream_ptr()), "sar_gin_sample_bwd_data_f32")


def gin_sample_eps_grad(x, dout, deps, F, V, N, scratch=None):
    """deps[0] = <x, dout> over the F x N V live elements (sar_gin_sample_eps_grad_f32); deps: one float32 on the device"""
    lib = L.load()
    assert deps.is_cuda and deps.dtype == torch.float32 and deps.numel() == 1, "deps must be one float32 on the device"
    if scratch is None:
        scratch = torch.empty(lib.sar_gin_sample_eps_grad_scratch_floats(F, V, N), dtype=torch.float32, device=x.device)
    check(lib.sar_gin_sample_eps_grad_f32(ptr(_f32(x)), x.stride(0), ptr(_f32(dout)), dout.stride(0), F, V, N, ptr(scratch), ptr(deps),
                                          stream_ptr()), "sar_gin_sample_eps_grad_f32")


# ------------------------------------------------------------------------------------------------ TemporalSampler (csrc/lstm.hip)
def _i32(t, shape):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
        "need a contiguous cuda int32 tensor of shape %s" % (tuple(shape),)
    return t


def lstm_fwd(zin, U, h, u, N, T, gates=None, c=None):
    """h [u][T N] of one Keras LSTM layer from zin [4u][T N] = kernel^T x + bias and U = recurrent_kernel (u, 4u), all T steps in one
    launch (sar_lstm_fwd_f32); time-major columns t N + n.  gates [4u][T N] (post-activation i, f, g, o) and c [u][T N] are saved
    when given (both or neither)."""
    assert U.is_contiguous() and tuple(U.shape) == (u, 4 * u), "U must be the contiguous (u, 4u) recurrent kernel"
    assert zin.shape[0] == 4 * u and h.shape[0] == u and (gates is None or gates.shape[0] == 4 * u) and (c is None or c.shape[0] == u)
    check(L.load().sar_lstm_fwd_f32(ptr(_f32(zin)), zin.stride(0), ptr(_f32(U)), ptr(_f32(h)), h.stride(0), ptr(_f32(gates)),
                                    gates.stride(0) if gates is not None else 0, ptr(_f32(c)), c.stride(0) if c is not None else 0,
                                    u, N, T, stream_ptr()), "sar_lstm_fwd_f32")


def lstm_bwd(dh, gates, c, U, dz, u, N, T):
    """dz [4u][T N] (the gradient at the pre-activations, rows i, f, c, o) from dh [u][T N] (the gradient arriving at h from above),
    the saved gates and c, and U: back-propagation through time in one launch (sar_lstm_bwd_f32)"""
    assert U.is_contiguous() and tuple(U.shape) == (u, 4 * u), "U must be the contiguous (u, 4u) recurrent kernel"
    assert dh.shape[0] == u and gates.shape[0] == 4 * u and c.shape[0] == u and dz.shape[0] == 4 * u
    check(L.load().sar_lstm_bwd_f32(ptr(_f32(dh)), dh.stride(0), ptr(_f32(gates)), gates.stride(0), ptr(_f32(c)), c.stride(0),
                                    ptr(_f32(U)), ptr(_f32(dz)), dz.stride(0), u, N, T, stream_ptr()), "sar_lstm_bwd_f32")


def topk_desc(scores, stride_n, stride_t, N, T, k, values, idx, inv):
    """per sequence the k best of scores[n stride_n + t stride_t], descending, equal scores in ascending frame index
    (sar_topk_desc_f32) -> values (N, k) float32, idx (N, k) int32, inv (N, T) int32 (j where frame t = idx[n, j], else -1)"""
    assert scores.is_cuda and scores.dtype == torch.float32
    assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and tuple(values.shape) == (N, k)
    check(L.load().sar_topk_desc_f32(ptr(scores), stride_n, stride_t, N, T, k, ptr(values), ptr(_i32(idx, (N, k))),
                                     ptr(_i32(inv, (N, T))), stream_ptr()), "sar_topk_desc_f32")


def frame_gather(x, idx, values, out):
    """out (N, C, k, V) = x (N, C, T, V) at the frames idx (N, k), scaled by values (N, k) (sar_frame_gather_f32)"""
    N, C, T, V = x.shape
    k = idx.shape[1]
    assert x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (N, C, k, V) and values.is_contiguous()
    assert tuple(values.shape) == (N, k)
    check(L.load().sar_frame_gather_f32(ptr(_f32(x)), ptr(_i32(idx, (N, k))), ptr(_f32(values)), ptr(_f32(out)), N, C, T, V, k,
                                        stream_ptr()), "sar_frame_gather_f32")


def frame_gather_bwd(x, dout, values, inv, dvalues, dscores, stride_n, stride_t, dx=None):
    """the gather's gradients (sar_frame_gather_bwd_f32): dvalues (N, k), dscores in the scores' strided layout, dx (N, C, T, V) when
    given; every element written once"""
    N, C, T, V = x.shape
    k = dout.shape[2]
    assert x.is_contiguous() and dout.is_contiguous() and tuple(dout.shape) == (N, C, k, V) and (dx is None or dx.is_contiguous())
    assert values.is_contiguous() and dvalues.is_contiguous() and tuple(values.shape) == (N, k) == tuple(dvalues.shape)
    assert dscores.is_cuda and dscores.dtype == torch.float32 and (dx is None or dx.shape == x.shape)
    check(L.load().sar_frame_gather_bwd_f32(ptr(_f32(x)), ptr(_f32(dout)), ptr(_f32(values)), ptr(_i32(inv, (N, T))), ptr(_f32(dvalues)),
                                            ptr(dscores), stride_n, stride_t, ptr(_f32(dx)), N, C, T, V, k, stream_ptr()),
          "sar_frame_gather_bwd_f32")


def lstm_pack(x, X):
    """X[v C + c][t N + n] = x[n, c, t, v] (sar_lstm_pack_f32): the LSTM stack's input matrix of a contiguous (N, C, T, V) tensor"""
    N, C, T, V = x.shape
    assert x.is_contiguous() and X.shape[0] == V * C
    check(L.load().sar_lstm_pack_f32(ptr(_f32(x)), ptr(_f32(X)), X.stride(0), N, C, T, V, stream_ptr()), "sar_lstm_pack_f32")


def lstm_unpack_add(X, x):
    """x[n, c, t, v] += X[v C + c][t N + n] (sar_lstm_unpack_add_f32)"""
    N, C, T, V = x.shape
    assert x.is_contiguous() and X.shape[0] == V * C
    check(L.load().sar_lstm_unpack_add_f32(ptr(_f32(X)), X.stride(0), ptr(_f32(x)), N, C, T, V, stream_ptr()), "sar_lstm_unpack_add_f32")


# ------------------------------------------------------------------------------------------------ graph isomorphism conv
def gin_adjacency(A, eps, table, scale, slice_scale=None, Km1=None, V=None):
    """table [Km1+1][V][V] (or None), scale[C] = 1 + eps, slice_scale[Km1+1] = (1, .., 1, 1 + eps) (or None)"""
    if A is not None:
        Km1, V = A.shape[0], A.shape[1]
    check(L.load().sar_gin_adjacency_f32(ptr(_f32(A)), Km1, V, ptr(_f32(eps)), ptr(_f32(table)), ptr(_f32(scale)), scale.numel(),
                                         ptr(_f32(slice_scale)), stream_ptr()), "sar_gin_adjacency_f32")


def graph_gather_sum(inp, tables, scale, K, F, V, out, add=None, k0=0):
    """out[m] = sum_k scale[k] (in[k F + m] gathered with slice k0 + k of `tables`) (+ add[m])"""
    n = out.shape[1]
    nz = (C.c_int32 * K)(*tables.nz[k0:k0 + K])
    check(L.load().sar_graph_gather_sum_f32(ptr(_f32(inp)), inp.stride(0), ptr(tables.idx[k0:]), ptr(tables.wt[k0:]),
                                            C.cast(nz, C.c_void_p), ptr(_f32(scale)),
                                            K, F, V, n, ptr(_f32(out)), out.stride(0), ptr(_f32(add)),
                                            add.stride(0) if add is not None else 0, stream_ptr()), "sar_graph_gather_sum_f32")


def graph_gather_expand(inp, tables, K, F, V, out, k0=0):
    """out[k F + m] = in[m] gathered with slice k0 + k of `tables`"""
    n = inp.shape[1]
    nz = (C.c_int32 * K)(*tables.nz[k0:k0 + K])
    check(L.load().sar_graph_gather_expand_f32(ptr(_f32(inp)), inp.stride(0), ptr(tables.idx[k0:]), ptr(tables.wt[k0:]),
                                               C.cast(nz, C.c_void_p), K, F, V, n, ptr(_f32(out)), out.stride(0), stream_ptr()),
          "sar_graph_gather_expand_f32")


def gin_sum_fwd(a, scale, shift, K, s_out, stats=False):
    Cc, n = s_out.shape
    partials, nparts = None, 0
    if stats:
        nparts = L.load().sar_gin_nparts(n)
        partials = torch.empty((Cc, nparts, 2), dtype=torch.float32, device=a.device)
    check(L.load().sar_gin_sum_fwd_f32(ptr(_f32(a)), a.stride(0), ptr(_f32(scale)), ptr(_f32(shift)), K, Cc, n, ptr(_f32(s_out)),
                                       s_out.stride(0), ptr(partials), stream_ptr()), "sar_gin_sum_fwd_f32")
    return (partials, nparts) if stats else None


def gin_bwd_reduce(ds, a, scale, shift, mean, K):
    Cc, n = ds.shape
    nparts = L.load().sar_gin_nparts(n)
    partials = torch.empty((K * Cc, nparts, 2), dtype=torch.float32, device=a.device)
    check(L.load().sar_gin_bwd_reduce_f32(ptr(_f32(ds)), ds.stride(0), ptr(_f32(a)), a.stride(0), ptr(_f32(scale)), ptr(_f32(shift)),
                                          ptr(_f32(mean)), K, Cc, n, ptr(partials), stream_ptr()), "sar_gin_bwd_reduce_f32")
    return partials, nparts


def gin_bwd_apply(ds, a, scale, shift, k, K, da):
    Cc, n = ds.shape
    check(L.load().sar_gin_bwd_apply_f32(ptr(_f32(ds)), ds.stride(0), ptr(_f32(a)), a.stride(0), ptr(_f32(scale)), ptr(_f32(shift)),
                                         ptr(_f32(k[0])), ptr(_f32(k[1])), ptr(_f32(k[2])), K, Cc, n, ptr(_f32(da)), da.stride(0),
                                         stream_ptr()), "sar_gin_bwd_apply_f32")


def gin_eps_grad(G, W, eps, deps):
    assert G.is_contiguous() and W.is_contiguous() and G.numel() == W.numel()
    check(L.load().sar_gin_eps_grad_f32(ptr(G), ptr(W), G.numel(), ptr(eps), ptr(deps), stream_ptr()), "sar_gin_eps_grad_f32")


def gin_eps_grad_bn(gamma, dgamma, rstd, bn_eps, eps, deps):
    """deps = bn_eps / (1 + eps) sum_c gamma dgamma rstd^2: d epsilon of a self slice in front of Conv -> BatchNorm, from that
    BatchNorm's backward (sar_gin_eps_grad_bn_f32); deps is left as it is when 1 + eps == 0"""
    check(L.load().sar_gin_eps_grad_bn_f32(ptr(_f32(gamma)), ptr(_f32(dgamma)), ptr(_f32(rstd)), gamma.numel(), bn_eps, ptr(eps),
                                           ptr(deps), stream_ptr()), "sar_gin_eps_grad_bn_f32")


# ================================================================================================ the layer wrappers
# Every wrapper below checks its operands with sar_amd/operands.py (O.on_gpu, O.cn_matrix, O.dense, O.view4) before L.load() is
# reached, allocates with _new and takes its 1x1 products from conv1x1_fwd / conv1x1_wgrad / conv1x1_dgrad above; only the size
# limits of its kernels are its own ("The layer wrappers")
def _new(dev, dtype=torch.float32):
    """shape -> an uninitialised tensor on `dev`"""
    return lambda *shape: torch.empty(shape, dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------------ ST-PGCN projection graph convolution
# csrc/pgc.hip (include/sar_hip.h: ProjectionGraphConv).  x / out / dout / dx: CN [64][B*P]; q: [32][B*P]
PGC_C, PGC_J = 64, 32
PGC_FWD_PART, PGC_DH_PART, PGC_BWD_PART, PGC_SAVED, PGC_DSAVED, PGC_SLAB = 2080, 2048, 4096, 11360, 2080, 8256


def _pgc_lds(B, P, **cn):
    """the row strides of the CN operands [64][B*P], each checked in turn as a float32 CUDA tensor, then as that matrix"""
    if B < 1 or P < 1:
        raise ValueError("ProjectionGraphConv needs B >= 1 and P >= 1 (got B = %d, P = %d)" % (B, P))
    lds = []
    for what, t in cn.items():
        O.on_gpu("ProjectionGraphConv", (t,))
        lds.append(O.cn_matrix(t, PGC_C, B * P, what))
    return lds


def pgc_forward(x, B, P, centers, variance, W, bias, out):
    """out = x + the projection graph convolution of x (models/stpgcn.py:23-47).  Returns (q [32][B*P], saved [B][PGC_SAVED]):
    what the backward pass needs (saved: S | zp | zn | g | h | A | qs | sum_j zp^2 per sample)."""
    ld, ld_out = _pgc_lds(B, P, x=x, out=out)
    lib, new = L.load(), _new(x.device)
    G = lib.sar_pgc_nparts(P)
    q, part, saved = new(PGC_J, B * P), new(B, G, PGC_FWD_PART), new(B, PGC_SAVED)
    check(lib.sar_pgc_assign_f32(ptr(x), ld, B, P, ptr(_f32(centers)), ptr(_f32(variance)), ptr(q), ptr(part), stream_ptr()),
          "sar_pgc_assign_f32")
    check(lib.sar_pgc_small_fwd_f32(ptr(part), B, G, ptr(centers), ptr(variance), ptr(_f32(W)), ptr(_f32(bias)), ptr(saved),
                                    stream_ptr()), "sar_pgc_small_fwd_f32")
    check(lib.sar_pgc_project_f32(ptr(x), ld, ptr(q), ptr(saved), B, P, ptr(out), ld_out, stream_ptr()),
          "sar_pgc_project_f32")
    return q, saved


def pgc_backward(x, dout, q, saved, B, P, centers, variance, W, dx, g_centers, g_variance, g_kernel_bias):
    """dx = the gradient w.r.t. x; g_centers / g_variance ([64][32]) and g_kernel_bias (the Conv1D kernel [64*64] followed by its
    bias [64], one contiguous range) are written, not accumulated.  Every sum runs in a fixed order."""
    ld, ld_dout, ld_dx = _pgc_lds(B, P, x=x, dout=dout, dx=dx)
    if not (g_kernel_bias.is_contiguous() and g_kernel_bias.numel() == PGC_C * PGC_C + PGC_C):
        raise ValueError("g_kernel_bias must be one contiguous range of %d elements (got shape %s, strides %s)"
                         % (PGC_C * PGC_C + PGC_C, tuple(g_kernel_bias.shape), tuple(g_kernel_bias.stride())))
    lib, new = L.load(), _new(x.device)
    G = lib.sar_pgc_nparts(P)
    part = new(B, G, PGC_DH_PART)
    check(lib.sar_pgc_bwd_reduce_f32(ptr(dout), ld_dout, ptr(q), B, P, ptr(part), stream_ptr()), "sar_pgc_bwd_reduce_f32")
    dsaved, slab = new(B, PGC_DSAVED), new(B, PGC_SLAB)
    check(lib.sar_pgc_small_bwd_f32(ptr(part), B, G, ptr(_f32(variance)), ptr(_f32(W)), ptr(saved), ptr(dsaved), ptr(slab), stream_ptr()),
          "sar_pgc_small_bwd_f32")
    cpart = new(B, G, PGC_BWD_PART)
    check(lib.sar_pgc_bwd_column_f32(ptr(x), ld, ptr(dout), ld_dout, ptr(q), ptr(saved), ptr(dsaved), ptr(_f32(centers)),
                                     ptr(variance), B, P, ptr(dx), ld_dx, ptr(cpart), stream_ptr()), "sar_pgc_bwd_column_f32")
    nwb = PGC_C * PGC_C + PGC_C
    sums = new(2 * PGC_BWD_PART)      # column partials | pooled slabs
    check(lib.sar_slab_reduce_f32(ptr(slab), B, PGC_SLAB, nwb, ptr(g_kernel_bias), stream_ptr()), "sar_slab_reduce_f32")
    check(lib.sar_slab_reduce_f32(ptr(slab) + 4 * nwb, B, PGC_SLAB, PGC_BWD_PART, ptr(sums) + 4 * PGC_BWD_PART, stream_ptr()),
          "sar_slab_reduce_f32")
    check(lib.sar_slab_reduce_f32(ptr(cpart), B * G, PGC_BWD_PART, PGC_BWD_PART, ptr(sums), stream_ptr()), "sar_slab_reduce_f32")
    check(lib.sar_pgc_param_grad_f32(ptr(sums), ptr(sums) + 4 * PGC_BWD_PART, ptr(variance), ptr(_f32(g_centers)), ptr(_f32(g_variance)),
                                     stream_ptr()), "sar_pgc_param_grad_f32")


# ------------------------------------------------------------------------------------------------ ST-PGCNP projection graph pooling
# csrc/pgpool.hip (include/sar_hip.h: ProjectionGraphPool).  x / dx: CN [C][B*P]; q / dq: [J][B*P]; centers / variance: C * J elements
PGPOOL_MAX = 512


def _pgpool_check(B, P, C, J, cn, dense, i32=()):
    """ValueError before the library is touched: sizes the kernels are not built for, then the `cn` operands (name -> CN matrix of
    B * P columns), then the `dense` ones (name -> contiguous tensor), then all of them and `i32` on the GPU in their dtype"""
    if not (1 <= C <= PGPOOL_MAX and 1 <= J <= PGPOOL_MAX):
        raise ValueError("ProjectionGraphPool is built for 1 <= C <= %d and 1 <= J <= %d (got C = %d, J = %d)" % (PGPOOL_MAX, PGPOOL_MAX, C, J))
    if B < 1 or P < 1:
        raise ValueError("ProjectionGraphPool needs B >= 1 and P >= 1 (got B = %d, P = %d)" % (B, P))
    for what, t in cn.items():
        O.cn_matrix(t, None, B * P, what)
    for what, t in dense.items():
        O.dense(t, None, what)
    O.on_gpu("ProjectionGraphPool", tuple(cn.values()) + tuple(dense.values()), i32)


def pgpool_forward(x, B, P, centers, variance):
    """ProjectionGraphPool forward (models/stpgcnp.py:22-38) of the CN matrix x [C][B*P] (may be a row-strided view).  Returns
    (zn (B, C, J), A_out (B, J, J), saved): saved = (q [J][B*P], clamp bits, zp (B, C, J), qs (B, J), n2 (B, C), tab (4, C, J)) is what
    pgpool_backward needs."""
    C, J = x.shape[0], centers.numel() // max(x.shape[0], 1)
    _pgpool_check(B, P, C, J, dict(x=x), dict(centers=centers, variance=variance))
    if centers.numel() != C * J or variance.numel() != C * J:
        raise ValueError("centers / variance must hold C * J = %d elements each" % (C * J))
    lib, new = L.load(), _new(x.device)
    q, tab, S, zn, A = new(J, B * P), new(4, C, J), new(B, C, J), new(B, C, J), new(B, J, J)
    qs, n2 = new(B, J), new(B, C)
    clamp = _new(x.device, torch.int32)(B * P, lib.sar_pgpool_clamp_words(J))
    st = stream_ptr()
    check(lib.sar_pgpool_prep_f32(ptr(centers), ptr(variance), C, J, ptr(tab), st), "sar_pgpool_prep_f32")
    check(lib.sar_pgpool_assign_f32(ptr(x), x.stride(0), B, P, C, J, ptr(centers), ptr(tab), ptr(q), q.stride(0), ptr(clamp), st),
          "sar_pgpool_assign_f32")
    check(lib.sar_pgpool_moment_f32(ptr(x), x.stride(0), ptr(q), q.stride(0), B, P, C, J, 0, ptr(S), st), "sar_pgpool_moment_f32")
    check(lib.sar_pgpool_rowsum_f32(ptr(q), q.stride(0), B, P, J, ptr(qs), st), "sar_pgpool_rowsum_f32")
    check(lib.sar_pgpool_normalize_f32(ptr(S), ptr(qs), ptr(centers), ptr(tab), B, C, J, ptr(zn), ptr(n2), st), "sar_pgpool_normalize_f32")
    check(lib.sar_pgpool_gram_f32(ptr(zn), B, C, J, ptr(A), st), "sar_pgpool_gram_f32")
    return zn, A, (q, clamp, S, qs, n2, tab)      # (S now holds zp)


def pgpool_backward(x, B, P, centers, zn, saved, dz, dA, dx, dcenters, dvariance):
    """Backward of pgpool_forward from dz (B, C, J) and dA (B, J, J) (either may be None = zero): dx [C][B*P], dcenters / dvariance
    (C * J elements each) are written.  Returns dl [J][B*P]."""
    q, clamp, zp, qs, n2, tab = saved
    C, J = x.shape[0], q.shape[0]
    dev, new = x.device, _new(x.device)
    if dz is None:
        dz = torch.zeros((B, C, J), dtype=torch.float32, device=dev)
    if dA is None:
        dA = torch.zeros((B, J, J), dtype=torch.float32, device=dev)
    dq = new(J, B * P)
    _pgpool_check(B, P, C, J, dict(x=x, q=q, dx=dx, dq=dq), dict(centers=centers, zn=zn, dz=dz, dA=dA, dcenters=dcenters,
                                                                 dvariance=dvariance), i32=(clamp,))
    if tuple(dz.shape) != (B, C, J) or tuple(dA.shape) != (B, J, J) or dcenters.numel() != C * J or dvariance.numel() != C * J:
        raise ValueError("dz must be (B, C, J), dA (B, J, J), dcenters / dvariance C * J elements")
    lib = L.load()
    st = stream_ptr()
    dzn, dS, dqs = new(B, C, J), new(B, C, J), new(B, J)
    check(lib.sar_pgpool_gram_bwd_f32(ptr(zn), ptr(dz), ptr(dA), B, C, J, ptr(dzn), st), "sar_pgpool_gram_bwd_f32")
    check(lib.sar_pgpool_normalize_bwd_f32(ptr(dzn), ptr(zn), ptr(zp), ptr(n2), ptr(qs), ptr(centers), ptr(tab), B, C, J, ptr(dS),
                                           ptr(dqs), st), "sar_pgpool_normalize_bwd_f32")
    check(lib.sar_pgpool_dq_f32(ptr(x), x.stride(0), ptr(dS), ptr(dqs), B, P, C, J, ptr(dq), dq.stride(0), st), "sar_pgpool_dq_f32")
    check(lib.sar_pgpool_softmax_bwd_f32(ptr(q), q.stride(0), ptr(clamp), B, P, J, ptr(dq), dq.stride(0), st), "sar_pgpool_softmax_bwd_f32")
    check(lib.sar_pgpool_dx_f32(ptr(x), x.stride(0), ptr(dS), ptr(q), q.stride(0), ptr(dq), dq.stride(0), ptr(tab), B, P, C, J, ptr(dx),
                                dx.stride(0), st), "sar_pgpool_dx_f32")
    M0, M1, M2 = dqs, dzn, new(B, C, J)           # (dqs and dzn have been consumed)
    check(lib.sar_pgpool_rowsum_f32(ptr(dq), dq.stride(0), B, P, J, ptr(M0), st), "sar_pgpool_rowsum_f32")
    check(lib.sar_pgpool_moment_f32(ptr(x), x.stride(0), ptr(dq), dq.stride(0), B, P, C, J, 0, ptr(M1), st), "sar_pgpool_moment_f32")
    check(lib.sar_pgpool_moment_f32(ptr(x), x.stride(0), ptr(dq), dq.stride(0), B, P, C, J, 1, ptr(M2), st), "sar_pgpool_moment_f32")
    check(lib.sar_pgpool_param_grad_f32(ptr(M0), ptr(M1), ptr(M2), ptr(dS), ptr(qs), ptr(zp), ptr(centers), ptr(tab), B, C, J,
                                        ptr(dcenters), ptr(dvariance), st), "sar_pgpool_param_grad_f32")
    return dq                                     # (holds dl)


# ------------------------------------------------------------------------------------------------ GPool top-k graph pooling
# csrc/gpool.hip (include/sar_hip.h: GPool).  x / out / their gradients are 4-D (N, C, T, W) tensors OR VIEWS whose two inner strides
# are (W, 1): the NCHW tensors of the modules, or the view X[:, :N*T*W].view(C, N, T, W).permute(1, 0, 2, 3) of an engine's CN matrix
GPOOL_VMAX, GPOOL_KMAX, GPOOL_NMAX = 64, 8, 65535


def gpool_keep(keeprate, V):
    """int(float32(keeprate) * float32(V)), the reference's `int(keeprate * tf.cast(V, float32))`"""
    import numpy as np
    keep = int(np.float32(keeprate) * np.float32(V))
    if not (0.0 < float(keeprate) <= 1.0) or keep < 1:
        raise ValueError("keeprate must be in (0, 1] and keep at least one of the V = %d vertices (got keeprate = %r: keep = %d)"
                         % (V, keeprate, keep))
    return keep


def _gpool_check(N, C, T, V, K):
    if not (1 <= V <= GPOOL_VMAX and 1 <= K <= GPOOL_KMAX):
        raise ValueError("GPool is built for 1 <= V <= %d and 1 <= K <= %d (got V = %d, K = %d)" % (GPOOL_VMAX, GPOOL_KMAX, V, K))
    if not (1 <= N <= GPOOL_NMAX and C >= 1 and T >= 1 and N * C * T * V < 1 << 31):
        raise ValueError("GPool is built for 1 <= N <= %d and fewer than 2^31 elements (got N = %d, C = %d, T = %d, V = %d)"
                         % (GPOOL_NMAX, N, C, T, V))


def gpool_forward(x, A, p, keeprate, out=None):
    """GPool forward (models/stgcn_debug.py:39-72) of x (N, C, T, V) -- a tensor or a strided view, see above --, A (N, K, V, V) and
    projection_vector p (C T elements).  Returns (out (N, C, T, keep), A_out (N, K, keep, keep), saved); `out` may be given as a view
    of the caller's buffer.  saved = (idx (N, keep) int32, pos (N, V) int32, y (N, V), s (N, keep), ph (C T), norm (2)) is what
    gpool_backward needs besides x, A and p."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise ValueError("x must be 4-D (N, C, T, V)")
    if not (isinstance(A, torch.Tensor) and A.dim() == 4):
        raise ValueError("A must be 4-D (N, K, V, V): expand a 3-D adjacency to (N, K, V, V)")
    N, C, T, V = x.shape
    K = A.shape[1]
    _gpool_check(N, C, T, V, K)
    keep = gpool_keep(keeprate, V)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    O.dense(A, (N, K, V, V), "A")
    if not (isinstance(p, torch.Tensor) and p.numel() == C * T):
        raise ValueError("projection_vector must hold C * T = %d elements" % (C * T))
    O.dense(p, None, "projection_vector")
    O.on_gpu("GPool", (x, A, p))
    new, newi = _new(x.device), _new(x.device, torch.int32)
    if out is None:
        out = new(N, C, T, keep)
    on, oc = O.view4(out, (N, C, T, keep), "out")
    O.on_gpu("GPool", (out,))
    lib = L.load()
    ph, norm, part = new(C * T), new(2), new(N, lib.sar_gpool_groups(C, T), V)
    y, s, idx, pos, A_out = new(N, V), new(N, keep), newi(N, keep), newi(N, V), new(N, K, keep, keep)
    st = stream_ptr()
    check(lib.sar_gpool_prep_f32(ptr(p), C * T, ptr(ph), ptr(norm), st), "sar_gpool_prep_f32")
    check(lib.sar_gpool_score_f32(ptr(x), sn, sc, ptr(ph), N, C, T, V, ptr(part), st), "sar_gpool_score_f32")
    check(lib.sar_gpool_select_f32(ptr(part), N, C, T, V, keep, ptr(y), ptr(idx), ptr(s), ptr(pos), st), "sar_gpool_select_f32")
    check(lib.sar_gpool_gather_f32(ptr(x), sn, sc, ptr(idx), ptr(s), N, C, T, V, keep, ptr(out), on, oc, st), "sar_gpool_gather_f32")
    check(lib.sar_gpool_adj_f32(ptr(A), ptr(idx), N, K, V, keep, ptr(A_out), st), "sar_gpool_adj_f32")
    return out, A_out, (idx, pos, y, s, ph, norm)


def gpool_backward(x, A, saved, dout, dA_out, dx=None):
    """Backward of gpool_forward from dout (N, C, T, keep; tensor or strided view) and dA_out (N, K, keep, keep); either may be None.
    Returns (dx, dp (C T), dA): dx / dp are None without dout, dA is None without dA_out.  dx may be given as a view of the caller's
    buffer; every element of it is written."""
    idx, pos, y, s, ph, norm = saved
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and isinstance(A, torch.Tensor) and A.dim() == 4):
        raise ValueError("x must be 4-D (N, C, T, V) and A 4-D (N, K, V, V)")
    N, C, T, V = x.shape
    K, keep = A.shape[1], idx.shape[1]
    _gpool_check(N, C, T, V, K)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    O.dense(A, (N, K, V, V), "A")
    O.dense(idx, (N, keep), "idx")
    O.dense(pos, (N, V), "pos")
    new = _new(x.device)
    dp = dA = None
    if dout is not None:
        dn, dc = O.view4(dout, (N, C, T, keep), "dout")
        if dx is not None:
            gn, gc = O.view4(dx, (N, C, T, V), "dx")
    if dA_out is not None:
        O.dense(dA_out, (N, K, keep, keep), "dA_out")
    O.on_gpu("GPool", (x, A, y, s, ph, norm) + tuple(t for t in (dout, dA_out, dx) if t is not None), (idx, pos))
    if dout is not None and dx is None:
        dx = new(N, C, T, V)
        gn, gc = O.view4(dx, (N, C, T, V), "dx")
    lib = L.load()
    st = stream_ptr()
    if dout is not None:
        part, dy, dphp, dph, dp = new(N, lib.sar_gpool_groups(C, T), keep), new(N, V), new(N, C * T), new(C * T), new(C * T)
        check(lib.sar_gpool_ds_f32(ptr(x), sn, sc, ptr(dout), dn, dc, ptr(idx), N, C, T, V, keep, ptr(part), st), "sar_gpool_ds_f32")
        check(lib.sar_gpool_dy_f32(ptr(part), ptr(s), ptr(idx), N, C, T, V, keep, ptr(dy), st), "sar_gpool_dy_f32")
        check(lib.sar_gpool_dx_f32(ptr(x), sn, sc, ptr(dout), dn, dc, ptr(pos), ptr(s), ptr(dy), ptr(ph), N, C, T, V, keep, ptr(dx), gn, gc,
                                   ptr(dphp), st), "sar_gpool_dx_f32")
        check(lib.sar_gpool_dp_f32(ptr(dphp), ptr(ph), ptr(norm), N, C * T, ptr(dph), ptr(dp), st), "sar_gpool_dp_f32")
    else:
        dx = None
    if dA_out is not None:
        dA = new(N, K, V, V)
        check(lib.sar_gpool_adj_bwd_f32(ptr(A), ptr(dA_out), ptr(idx), ptr(pos), N, K, V, keep, ptr(dA), st), "sar_gpool_adj_bwd_f32")
    return dx, dp, dA


# ------------------------------------------------------------------------------------------------ TemporalAttention
# csrc/tattn.hip (include/sar_hip.h: TemporalAttention).  x / out / dout / dx are 4-D (N, C, T, V) tensors or views whose two inner
# strides are (V, 1) (O.view4).  params = [kernel_1, bias_1, .., kernel_L, bias_L] in the Keras layouts, kernel_i (in, units),
# in_1 = V C with row v C + c, units_L = 1.  The hidden activations are CN matrices [units][N T]
TATTN_UMAX, TATTN_VMAX = 128, 64
TATTN_RELU, TATTN_SIGMOID = 0, 1


def _tattn_check(x, params):
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise ValueError("x must be 4-D (N, C, T, V)")
    N, C, T, V = x.shape
    if min(N, C, T, V) < 1 or V > TATTN_VMAX:
        raise ValueError("TemporalAttention is built for a non-empty x with V <= %d (got %s)" % (TATTN_VMAX, tuple(x.shape)))
    if N * T >= 1 << 22 or N * C * T * V >= 1 << 31:
        raise ValueError("TemporalAttention is built for N T < 2^22 and fewer than 2^31 elements (got %s)" % (tuple(x.shape),))
    params = list(params)
    if not params or len(params) % 2 or not all(isinstance(p, torch.Tensor) for p in params):
        raise ValueError("params must be [kernel_1, bias_1, .., kernel_L, bias_L] with L >= 1")
    features = V * C
    for i in range(0, len(params), 2):
        kernel, bias = params[i], params[i + 1]
        if not (kernel.dim() == 2 and kernel.shape[0] == features and tuple(bias.shape) == (kernel.shape[1],)
                and kernel.is_contiguous() and bias.is_contiguous()):
            raise ValueError("layer %d: need a contiguous kernel (%d, units) and bias (units), got %s and %s"
                             % (i // 2, features, tuple(kernel.shape), tuple(bias.shape)))
        features = kernel.shape[1]
        if not 1 <= features <= TATTN_UMAX:
            raise ValueError("layer %d: the kernels are built for 1 <= units <= %d (got %d)" % (i // 2, TATTN_UMAX, features))
    if features != 1:
        raise ValueError("the last layer must have one unit (Dense(1, sigmoid)), got %d" % features)
    return N, C, T, V, params


def tattn_forward(x, params, out=None):
    """TemporalAttention forward (models/stgcn.py:75-85) of x (N, C, T, V), a tensor or a strided view.  Returns (out, saved); `out` may
    be given as a view of the caller's buffer.  saved = (a (N T), h_1 (units_1, N T), .., h_{L-1}): the gate and the hidden
    activations, what tattn_backward needs besides x and params."""
    N, C, T, V, params = _tattn_check(x, params)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    if out is not None:
        on, oc = O.view4(out, (N, C, T, V), "out")
    O.on_gpu("TemporalAttention", [x] + params + ([out] if out is not None else []))
    new, n, nl = _new(x.device), N * T, len(params) // 2
    if out is None:
        out = new(N, C, T, V)
        on, oc = O.view4(out, (N, C, T, V), "out")
    lib, st, geo = L.load(), stream_ptr(), column_geometry(N, T)      # (the later layers: 1x1 products over the N T columns)
    u = params[0].shape[1]
    h = new(u, n)
    check(lib.sar_tattn_score_f32(ptr(x), sn, sc, ptr(params[0]), ptr(params[1]), N, C, T, V, u, TATTN_SIGMOID if nl == 1 else TATTN_RELU,
                                  ptr(h), n, st), "sar_tattn_score_f32")
    hs = []
    for i in range(1, nl):
        hs.append(h)
        h = conv1x1_fwd(h, params[2 * i], params[2 * i + 1], geo)
        check(lib.sar_tattn_act_f32(ptr(h), n, h.shape[0], n, TATTN_SIGMOID if i == nl - 1 else TATTN_RELU, st), "sar_tattn_act_f32")
    a = h.view(n)
    check(lib.sar_tattn_scale_f32(ptr(x), sn, sc, ptr(a), N, C, T, V, ptr(out), on, oc, st), "sar_tattn_scale_f32")
    return out, (a,) + tuple(hs)


def tattn_backward(x, saved, params, dout, need_dx=True, dx=None, keep=None):
    """Backward of tattn_forward from dout (N, C, T, V; tensor or strided view).  Returns (dx | None, grads): grads in the order of
    params; dx (every element written; may be given as a view of the caller's buffer) only with need_dx -- without it the input
    gradient's product is not launched.  keep: a dict that receives the gradients at the last and the first pre-activation, "dz_L"
    (1, N T) and "dz_1" (units_1, N T), for the tests."""
    N, C, T, V, params = _tattn_check(x, params)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    dn, dc = O.view4(dout, (N, C, T, V), "dout")
    if need_dx and dx is not None:
        gn, gc = O.view4(dx, (N, C, T, V), "dx")
    n, nl = N * T, len(params) // 2
    a, hs = saved[0], list(saved[1:])
    if len(hs) != nl - 1 or a.numel() != n or any(tuple(h.shape) != (params[2 * i].shape[1], n) for i, h in enumerate(hs)):
        raise ValueError("saved does not belong to these params and this x")
    O.on_gpu("TemporalAttention", [x, dout, a] + hs + params + ([dx] if need_dx and dx is not None else []))
    new = _new(x.device)
    lib, st, geo = L.load(), stream_ptr(), column_geometry(N, T)
    dz = new(1, n)
    check(lib.sar_tattn_dscore_f32(ptr(x), sn, sc, ptr(dout), dn, dc, ptr(a), N, C, T, V, ptr(dz), st), "sar_tattn_dscore_f32")
    grads = [None] * len(params)
    if keep is not None:
        keep["dz_L"] = dz
    for i in range(nl - 1, 0, -1):
        kernel, h = params[2 * i], hs[i - 1]
        dW, grads[2 * i + 1] = conv1x1_wgrad(h, dz, geo)
        grads[2 * i] = dW.view(kernel.shape)
        dz = conv1x1_dgrad(dz, kernel, geo)
        check(lib.sar_tattn_dact_f32(ptr(h), n, ptr(dz), n, kernel.shape[0], n, st), "sar_tattn_dact_f32")
    if keep is not None:
        keep["dz_1"] = dz
    kernel = params[0]
    u, size = kernel.shape[1], kernel.numel() + kernel.shape[1]
    nslab = lib.sar_tattn_wgrad_slabs(N, C, T, V)
    slab, flat = new(nslab, size), new(size)
    check(lib.sar_tattn_wgrad_f32(ptr(x), sn, sc, ptr(dz), n, N, C, T, V, u, ptr(slab), nslab, st), "sar_tattn_wgrad_f32")
    check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(flat), st), "sar_slab_reduce_f32")
    grads[0], grads[1] = flat[:kernel.numel()].view(kernel.shape), flat[kernel.numel():]
    if not need_dx:
        return None, grads
    if dx is None:
        dx = new(N, C, T, V)
        gn, gc = O.view4(dx, (N, C, T, V), "dx")
    check(lib.sar_tattn_dx_f32(ptr(dout), dn, dc, ptr(a), ptr(kernel), ptr(dz), n, N, C, T, V, u, ptr(dx), gn, gc, st), "sar_tattn_dx_f32")
    return dx, grads


# ------------------------------------------------------------------------------------------------ AdaptiveAdjacency
# csrc/adjattn.hip (include/sar_hip.h: AdaptiveAdjacency).  X / dX: CN matrices [C][ld] with columns (n, t, v) -- the modules' to_cn(x)
# or an engine's own matrix (a row-strided view with N T V live columns); A (K, V, V); the kernels in the Keras layout (1, 1, C, K Ce)
# (or (C, K Ce)), channel k Ce + e of subset k; phi_bias (K Ce).  theta and phi are ONE 1x1 product on the stacked kernel [C][2 K Ce]
# (theta's columns, then phi's; zeros in the bias of theta's half) per pass: conv1x1_fwd / conv1x1_wgrad / conv1x1_dgrad.
ADJATTN_VMAX, ADJATTN_KMAX, ADJATTN_EMAX = 32, 4, 512


def _adjattn_check(X, N, T, V, A, theta_kernel, phi_kernel, phi_bias=None, **dense):
    """ValueError before the library is touched -> (C, K, Ce); dense: further contiguous operands by name"""
    rest = dict(A=A, theta_kernel=theta_kernel, phi_kernel=phi_kernel, **({} if phi_bias is None else dict(phi_bias=phi_bias)), **dense)
    if not all(isinstance(t, torch.Tensor) for t in (X, *rest.values())):
        raise ValueError("AdaptiveAdjacency operands must be tensors")
    if min(N, T, V) < 1:
        raise ValueError("AdaptiveAdjacency needs N, T, V >= 1 (got N = %d, T = %d, V = %d)" % (N, T, V))
    O.cn_matrix(X, None, N * T * V, "X")
    C = X.shape[0]
    if not (A.dim() == 3 and tuple(A.shape[1:]) == (V, V)):
        raise ValueError("A must be (K, V, V) = (K, %d, %d), got %s" % (V, V, tuple(A.shape)))
    K = A.shape[0]
    if not (1 <= V <= ADJATTN_VMAX and 1 <= K <= ADJATTN_KMAX):
        raise ValueError("AdaptiveAdjacency is built for 1 <= V <= %d and 1 <= K <= %d (got V = %d, K = %d)" % (ADJATTN_VMAX, ADJATTN_KMAX, V, K))
    kce = theta_kernel.shape[-1] if theta_kernel.dim() >= 2 else 0
    for name, kernel in (("theta_kernel", theta_kernel), ("phi_kernel", phi_kernel)):
        if not (kernel.dim() in (2, 4) and kernel.numel() == C * kce and tuple(kernel.shape[-2:]) == (C, kce)):
            raise ValueError("%s must be (1, 1, C, K Ce) = (1, 1, %d, %d), got %s" % (name, C, kce, tuple(kernel.shape)))
    if not (1 <= kce <= ADJATTN_EMAX and kce % K == 0):
        raise ValueError("AdaptiveAdjacency is built for 1 <= K Ce <= %d, a multiple of K = %d (got %d)" % (ADJATTN_EMAX, K, kce))
    if phi_bias is not None and tuple(phi_bias.shape) != (kce,):
        raise ValueError("phi_bias must be (K Ce) = (%d), got %s" % (kce, tuple(phi_bias.shape)))
    if N * T * V >= 1 << 22 or N * K > 65535:
        raise ValueError("AdaptiveAdjacency is built for N T V < 2^22 columns (the 1x1 product) and N K <= 65535 (got N = %d, T = %d, V = %d, "
                         "K = %d)" % (N, T, V, K))
    for what, t in rest.items():
        O.dense(t, None, what)
    O.on_gpu("AdaptiveAdjacency", (X, *rest.values()))
    return C, K, kce // K


def _adjattn_stacked(theta_kernel, phi_kernel, C):
    return torch.cat([theta_kernel.reshape(C, -1), phi_kernel.reshape(C, -1)], dim=1)


def adjattn_forward(X, N, T, V, A, theta_kernel, phi_kernel, phi_bias, keep=None):
    """A_eff[n, k] = A[k] + softmax_v(theta_k(x_n)^T phi_k(x_n) / (Ce T)) of the CN matrix X [C][ld].  Returns (A_eff (N, K, V, V), saved):
    saved = (E [2 K Ce][N T V]: theta's rows, then phi's; P (N, K, V, V)) is what adjattn_backward needs besides X and the kernels.
    keep: a dict that receives the logits "S" (N, K, V, V), for the tests."""
    C, K, Ce = _adjattn_check(X, N, T, V, A, theta_kernel, phi_kernel, phi_bias)
    new, kce = _new(X.device), K * Ce
    lib, st = L.load(), stream_ptr()
    bias = torch.cat([torch.zeros(kce, dtype=torch.float32, device=X.device), phi_bias])
    E = conv1x1_fwd(X, _adjattn_stacked(theta_kernel, phi_kernel, C), bias, dict(B=N, V=V, T_src=T, T_out=T))
    S, P, A_eff = new(N, K, V, V), new(N, K, V, V), new(N, K, V, V)
    nslab = lib.sar_adjattn_sim_slabs(Ce, T, V)
    slab = new(nslab, N * K * V * V) if nslab > 1 else None
    check(lib.sar_adjattn_sim_f32(ptr(E), ptr(E[kce:]), E.stride(0), N, K, Ce, T, V, ptr(S), ptr(slab), nslab, st), "sar_adjattn_sim_f32")
    check(lib.sar_adjattn_softmax_f32(ptr(S), ptr(A), N, K, V, ptr(P), ptr(A_eff), st), "sar_adjattn_softmax_f32")
    if keep is not None:
        keep["S"] = S
    return A_eff, (E, P)


def adjattn_backward(X, N, T, V, saved, theta_kernel, phi_kernel, dA_eff, need_dx=True, need_dA=True, keep=None):
    """Backward of adjattn_forward from dA_eff (N, K, V, V).  Returns (dX [C][N T V] | None, dtheta_kernel, dphi_kernel, dphi_bias,
    dA (K, V, V) | None); without need_dx the input gradient's product is not launched, without need_dA the sum over the samples is not.
    keep: a dict that receives "dS" (N, K, V, V) and "dE" [2 K Ce][N T V] (dtheta's rows, then dphi's), for the tests."""
    E, P = saved
    if not (isinstance(P, torch.Tensor) and P.dim() == 4 and isinstance(dA_eff, torch.Tensor) and tuple(dA_eff.shape) == tuple(P.shape)):
        raise ValueError("dA_eff must have the shape of the saved P, (N, K, V, V)")
    if not (isinstance(E, torch.Tensor) and isinstance(theta_kernel, torch.Tensor) and theta_kernel.dim() >= 2 and P.shape[0] == N
            and tuple(E.shape) == (2 * theta_kernel.shape[-1], N * T * V)):
        raise ValueError("saved does not belong to these kernels and this X")
    C, K, Ce = _adjattn_check(X, N, T, V, P[0], theta_kernel, phi_kernel, E=E, P=P, dA_eff=dA_eff)
    kce, n, new = K * Ce, N * T * V, _new(X.device)
    lib, st, geo = L.load(), stream_ptr(), dict(B=N, V=V, T_src=T, T_out=T)
    dS, dA, dE = new(N, K, V, V), (new(K, V, V) if need_dA else None), new(2 * kce, n)
    check(lib.sar_adjattn_softmax_bwd_f32(ptr(P), ptr(dA_eff), N, K, V, ptr(dS), ptr(dA), st), "sar_adjattn_softmax_bwd_f32")
    check(lib.sar_adjattn_dembed_f32(ptr(dS), ptr(E), ptr(E[kce:]), n, N, K, Ce, T, V, ptr(dE), ptr(dE[kce:]), n, st), "sar_adjattn_dembed_f32")
    if keep is not None:
        keep["dS"], keep["dE"] = dS, dE
    dW, db = conv1x1_wgrad(X, dE, geo)
    dW = dW.view(C, 2 * kce)
    dtk, dpk = dW[:, :kce].contiguous().view(theta_kernel.shape), dW[:, kce:].contiguous().view(phi_kernel.shape)
    dX = conv1x1_dgrad(dE, _adjattn_stacked(theta_kernel, phi_kernel, C), geo) if need_dx else None
    return dX, dtk, dpk, db[kce:], dA


# ------------------------------------------------------------------------------------------------ TemporalConv
# csrc/tconv.hip (include/sar_hip.h: TemporalConv).  x / dx (N, C, T, V) and out / dout (N, M, T_out, V) are 4-D tensors or views whose
# two inner strides are (V, 1) (O.view4): NCHW tensors and the view of an engine's CN matrix run the same kernels.  kernel: the Keras
# kernel (k, 1, C, M), contiguous; bias (M) or None.
TCONV_KMAX, TCONV_DMAX, TCONV_CMAX, TCONV_VMAX = 9, 8, 512, 64


def tconv_geometry(T, k, s, d, padding):
    """(T_out, pad) of a temporal convolution of T frames with k taps, stride s and dilation d.  padding="same": TensorFlow's SAME with
    the dilated extent (the odd frame of padding goes behind; at k = 9, d = 1 this is sar_amd.stgcn.same_pad); padding=p (an int):
    PyTorch's symmetric padding of p frames."""
    T, k, s, d = int(T), int(k), int(s), int(d)
    if min(T, k, s, d) < 1:
        raise ValueError("tconv_geometry needs T, k, s, d >= 1 (got %d, %d, %d, %d)" % (T, k, s, d))
    if padding == "same":
        T_out = -(-T // s)
        return T_out, max((T_out - 1) * s + (k - 1) * d + 1 - T, 0) // 2
    if isinstance(padding, bool) or not isinstance(padding, int) or padding < 0:
        raise ValueError("padding must be \"same\" or a number of frames >= 0 (got %r)" % (padding,))
    T_out = (T + 2 * padding - d * (k - 1) - 1) // s + 1
    if T_out < 1:
        raise ValueError("no output frame: T = %d, k = %d, d = %d with padding %d" % (T, k, d, padding))
    return T_out, padding


def tconv_limits(k, d, s, pad=0, C=1, M=1, V=1, N=1):
    """ValueError for what csrc/tconv.hip is not built for"""
    if not (1 <= k <= TCONV_KMAX and 1 <= d <= TCONV_DMAX and s in (1, 2) and 0 <= pad <= (k - 1) * d):
        raise ValueError("TemporalConv is built for 1 <= kernel_size <= %d, 1 <= dilation <= %d, stride 1 or 2 and 0 <= pad <= (k - 1) d "
                         "(got kernel_size = %d, dilation = %d, stride = %d, pad = %d)" % (TCONV_KMAX, TCONV_DMAX, k, d, s, pad))
    if not (1 <= C <= TCONV_CMAX and 1 <= M <= TCONV_CMAX and 1 <= V <= TCONV_VMAX and 1 <= N <= 65535):
        raise ValueError("TemporalConv is built for 1 <= C, filters <= %d, 1 <= V <= %d and 1 <= N <= 65535 (got C = %d, filters = %d, V = %d, "
                         "N = %d)" % (TCONV_CMAX, TCONV_VMAX, C, M, V, N))


def _tconv_check(x_shape, M, T_out, kernel, bias, s, d, pad):
    """every limit of the three entry points -> (N, C, T, V, k); kernel None: the weight gradient, which takes k from M = (k, M)"""
    if len(x_shape) != 4:
        raise ValueError("x must be 4-D (N, C, T, V), got shape %s" % (tuple(x_shape),))
    N, C, T, V = (int(v) for v in x_shape)
    if kernel is not None:
        if not (torch.is_tensor(kernel) and kernel.dim() == 4 and kernel.shape[1] == 1 and kernel.shape[2] == C):
            raise ValueError("kernel must be the Keras kernel (k, 1, C, filters) = (k, 1, %d, filters), got %s"
                             % (C, tuple(kernel.shape) if torch.is_tensor(kernel) else type(kernel).__name__))
        k, M = int(kernel.shape[0]), int(kernel.shape[3])
        O.dense(kernel, None, "kernel")
    else:
        k, M = M
    s, d, pad, T_out = int(s), int(d), int(pad), int(T_out)
    if min(N, C, T, V, M, T_out) < 1:
        raise ValueError("TemporalConv needs a non-empty x, filters >= 1 and T_out >= 1 (got x %s, filters = %d, T_out = %d)" % (tuple(x_shape), M, T_out))
    tconv_limits(k, d, s, pad, C, M, V, N)
    if N * C * T * V >= 1 << 31 or N * M * T_out * V >= 1 << 31:
        raise ValueError("TemporalConv is built for fewer than 2^31 elements per tensor (got x %s, filters = %d, T_out = %d)" % (tuple(x_shape), M, T_out))
    if (T_out - 1) * s + (k - 1) * d - pad > T + pad:
        raise ValueError("T_out = %d reads past what pad = %d allows (T = %d, kernel_size = %d, dilation = %d, stride = %d)" % (T_out, pad, T, k, d, s))
    if bias is not None:
        O.dense(bias, (M,), "bias")
    return N, C, T, V, k, M


def tconv_forward(x, kernel, bias, stride, dilation, pad, T_out, out=None):
    """out[n,m,to,v] = bias[m] + sum_{j,c} kernel[j,0,c,m] x[n, c, to stride + j dilation - pad, v] (x is 0 outside [0, T)) of
    x (N, C, T, V), a tensor or a strided view; bias may be None.  Returns out (N, M, T_out, V), which may be given as a view of the
    caller's buffer.  One launch."""
    if not torch.is_tensor(x):
        raise ValueError("x must be a tensor")
    N, C, T, V, k, M = _tconv_check(x.shape, None, T_out, kernel, bias, stride, dilation, pad)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    if out is not None:
        on, oc = O.view4(out, (N, M, T_out, V), "out")
    O.on_gpu("TemporalConv", [x, kernel] + [t for t in (bias, out) if t is not None])
    if out is None:
        out = torch.empty((N, M, T_out, V), dtype=torch.float32, device=x.device)
        on, oc = O.view4(out, (N, M, T_out, V), "out")
    flops, nbytes = 2.0 * M * C * k * N * T_out * V, 4.0 * (N * C * T * V + N * M * T_out * V + k * C * M)
    with profiler.region("tconv_fwd", flops, nbytes):
        check(L.load().sar_tconv_fwd_f32(ptr(x), sn, sc, ptr(kernel), ptr(bias), N, C, M, T, T_out, V, k, int(dilation), int(stride), int(pad),
                                         ptr(out), on, oc, stream_ptr()), "sar_tconv_fwd_f32")
    return out


def tconv_backward_data(dout, kernel, T, stride, dilation, pad, dx=None):
    """dx (N, C, T, V) of tconv_forward from dout (N, M, T_out, V), a tensor or a strided view; every element of dx is written, and dx
    may be given as a view of the caller's buffer.  Two launches: the (k, M, C) image of the kernel, the product."""
    if not (torch.is_tensor(dout) and dout.dim() == 4 and torch.is_tensor(kernel) and kernel.dim() == 4):
        raise ValueError("dout must be 4-D (N, filters, T_out, V) and kernel (k, 1, C, filters)")
    N, Md, T_out, V = dout.shape
    if kernel.shape[3] != Md:
        raise ValueError("dout has %d channels, the kernel %d filters" % (Md, kernel.shape[3]))
    N, C, T, V, k, M = _tconv_check((N, kernel.shape[2], T, V), None, T_out, kernel, None, stride, dilation, pad)
    dn, dc = O.view4(dout, (N, M, T_out, V), "dout")
    if dx is not None:
        gn, gc = O.view4(dx, (N, C, T, V), "dx")
    O.on_gpu("TemporalConv", [dout, kernel] + ([dx] if dx is not None else []))
    if dx is None:
        dx = torch.empty((N, C, T, V), dtype=torch.float32, device=dout.device)
        gn, gc = O.view4(dx, (N, C, T, V), "dx")
    kt = torch.empty((k, M, C), dtype=torch.float32, device=dout.device)
    transpose(kernel, kt, k, C, M)
    flops, nbytes = 2.0 * M * C * k * N * T_out * V, 4.0 * (N * C * T * V + N * M * T_out * V + k * C * M)
    with profiler.region("tconv_bwd_data", flops, nbytes):
        check(L.load().sar_tconv_bwd_data_f32(ptr(dout), dn, dc, ptr(kt), N, C, M, T, T_out, V, k, int(dilation), int(stride), int(pad), ptr(dx),
                                              gn, gc, stream_ptr()), "sar_tconv_bwd_data_f32")
    return dx


def tconv_wgrad(x, dout, kernel_size, stride, dilation, pad):
    """(dkernel (k, 1, C, M), dbias (M)) of tconv_forward from x (N, C, T, V) and dout (N, M, T_out, V), tensors or strided views.  Two
    launches: the slabs' partials, their sum in slab order."""
    if not (torch.is_tensor(x) and x.dim() == 4 and torch.is_tensor(dout) and dout.dim() == 4):
        raise ValueError("x must be 4-D (N, C, T, V) and dout 4-D (N, filters, T_out, V)")
    M, T_out = int(dout.shape[1]), int(dout.shape[2])
    N, C, T, V, k, M = _tconv_check(x.shape, (int(kernel_size), M), T_out, None, None, stride, dilation, pad)
    sn, sc = O.view4(x, (N, C, T, V), "x")
    dn, dc = O.view4(dout, (N, M, T_out, V), "dout")
    O.on_gpu("TemporalConv", [x, dout])
    lib, st, size = L.load(), stream_ptr(), k * C * M + M
    nslab = lib.sar_tconv_wgrad_slabs(N, C, M, T_out, V)
    if nslab < 1:
        check(nslab or -1, "sar_tconv_wgrad_slabs")
    slab = torch.empty((nslab, size), dtype=torch.float32, device=x.device)
    flat = torch.empty(size, dtype=torch.float32, device=x.device)
    flops, nbytes = 2.0 * M * C * k * N * T_out * V, 4.0 * (N * C * T * V + N * M * T_out * V + k * C * M)
    with profiler.region("tconv_wgrad", flops, nbytes):
        check(lib.sar_tconv_wgrad_f32(ptr(x), sn, sc, ptr(dout), dn, dc, N, C, M, T, T_out, V, k, int(dilation), int(stride), int(pad), ptr(slab),
                                      nslab, st), "sar_tconv_wgrad_f32")
        check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(flat), st), "sar_slab_reduce_f32")
    return flat[:k * C * M].view(k, 1, C, M), flat[k * C * M:]


# ------------------------------------------------------------------------------------------------ ResNet-18 ops
def _shape_tag(geo):
    """SAR_PROFILE_SHAPES=1 (diagnostic, tools/pathb_layers.py): one profiler bucket per layer geometry"""
    if not _PROFILE_SHAPES:
        return ""
    return " Kc%d M%d %dx%d->%dx%d s%d" % (geo["Kc"], geo["M"], geo["H_src"], geo["W_src"], geo["H_out"], geo["W_out"], geo["stride"])


def _conv2d_desc(src, *, B, Kc, M, H_src, W_src, H_out, W_out, KH, KW, stride, pad, transposed=False, pro=None,
                 pro_relu=False):
    d = L.Conv2dDesc()
    d.transposed, d.B, d.Kc, d.M = int(transposed), B, Kc, M
    d.H_src, d.W_src, d.H_out, d.W_out = H_src, W_src, H_out, W_out
    d.KH, d.KW, d.stride, d.pad, d.pro_relu = KH, KW, stride, pad, int(pro_relu)
    d.src, d.ld_src = ptr(_f32(src)), src.stride(0)
    if pro is not None:
        d.pro_scale, d.pro_shift = ptr(_f32(pro[0])), ptr(_f32(pro[1]))
    return d


def conv2d_split_applicable(*, KH, KW, stride, pad, Kc, M, H_src, W_src, H_out, W_out, aux_even_pixels=False, transposed=False,
                            epi=None, **_):
    """shapes csrc/conv2d_split.hip is built for: 3x3 / stride 1 / pad 1 (forward and data gradient; windows of <= 512 staged pixels)
    and the 3x3 / stride 2 / pad 1 DATA GRADIENT onto an image of exactly twice the size; the others stay fp32"""
    if KH == 3 and KW == 3 and stride == 2 and pad == 1 and transposed:
        if not (H_out == 2 * H_src and W_out == 2 * W_src and 16 <= Kc <= 512 and M % 8 == 0 and W_src <= 128):
            return False
        if aux_even_pixels and epi != L.SAR_EPI_ADD:
            return False
        cpix = H_src * W_src
        rw = (128 // cpix) * (H_src + 1) * (W_src + 1) if cpix <= 64 else (min(H_src, 128 // W_src) + 1) * (W_src + 1)
        return rw <= 256
    if not (KH == 3 and KW == 3 and stride == 1 and pad == 1 and H_src == H_out and W_src == W_out):
        return False
    if not (8 <= Kc <= 512 and M % 8 == 0 and not aux_even_pixels):
        return False
    opix = H_out * W_out
    rw = (256 // opix) * (H_out + 2) * (W_out + 2) if opix <= 128 else (min(H_out, 256 // W_out) + 2) * (W_out + 2) if W_out <= 256 else 1 << 30
    return rw <= 512


def _pack_split_conv2d(W, w_stride_tap, w_stride_c, Kc, M, arith, transposed):
    """one 3x3 tensor stored (tap, c, m), packed on the spot (kernel tests): (image, w_bound).  transposed: W is the DATA-GRADIENT
    operand layout (tap, m, c) of the forward tensor as the fp32 kernel takes it (element (tap, c', m') of the call = weight of
    forward tap `tap`); the stride-1 split kernel (transposed="mirror") wants the mirrored taps: item element (tap, c', m') =
    W[8 - tap][c'][m']; the stride-2 data gradient addresses the forward taps directly (no mirroring)."""
    if transposed == "mirror":
        return _pack_split_single(W, -w_stride_tap, w_stride_c, 9, Kc, M, arith, 8 * w_stride_tap)
    return _pack_split_single(W, w_stride_tap, w_stride_c, 9, Kc, M, arith)


def conv2d_gemm_route(split, *, aux_even_pixels=False, epi=L.SAR_EPI_NONE, **geo):
    """the kernel of a conv2d_gemm call: the split arithmetic (sar_conv2d_gemm_split: bf16x6 / f16x3a on the shapes of
    conv2d_split_applicable()) or None (sar_conv2d_gemm_f32).  `split`: "default" = DEFAULT_SPLIT.  No library, no tensor."""
    if split == "default":
        split = DEFAULT_SPLIT
    if split in ("f16x3a", "bf16x6") and conv2d_split_applicable(aux_even_pixels=aux_even_pixels, epi=epi, **geo):
        return split
    return None


def conv2d_gemm(src, out, W, w_stride_tap, w_stride_c, *, epi=L.SAR_EPI_NONE, aux=None, aux_affine=None, aux_mean=None,
                aux_even_pixels=False, ctx=None, split="default", packed=None, bounds=None, kslab=None, **geo):
    """sar_conv2d_gemm_f32 -- or, with split="f16x3a" / "bf16x6" on the shapes conv2d_split_applicable() names, the fp32-accurate
    split arithmetic on the fp16 / bf16 matrix pipe (sar_conv2d_gemm_split; `packed` = the PackedSplitWeights image of the launch's
    view of the weights or None = pack here from W; bounds = (src_bound, w_bound) cells, None = computed here by device kernels).
    Returns (partials, nparts) when the epilogue reduces.  aux_even_pixels: SAR_C2D_AUX_EVEN_PIXELS
    (aux is the compact data gradient of the parallel 1x1 / stride 2 convolution, added at the even pixels only).
    ctx: an L.Context whose side streams the call may fan out over (None: the current stream only).
    kslab: a callable nfloats -> flat float32 tensor that provides the K-split workspace (None: torch.empty here)."""
    lib = L.load()
    split = conv2d_gemm_route(split, aux_even_pixels=aux_even_pixels, epi=epi, **geo)
    d = _conv2d_desc(src, **geo)
    d.ctx = ctx.handle if ctx is not None else None
    d.flags = L.SAR_C2D_AUX_EVEN_PIXELS if aux_even_pixels else 0
    d.out, d.ld_out = ptr(_f32(out)), out.stride(0)
    d.W, d.w_stride_tap, d.w_stride_c, d.epi = ptr(_f32(W)), w_stride_tap, w_stride_c, epi
    if aux is not None:
        d.aux, d.ld_aux = ptr(_f32(aux)), aux.stride(0)
    if aux_affine is not None:
        d.aux_scale, d.aux_shift = ptr(_f32(aux_affine[0])), ptr(_f32(aux_affine[1]))
    d.aux_mean = ptr(_f32(aux_mean))
    partials, nparts = None, 0
    if split:      # small feature maps: workspace of the K-split (sar_hip.h), 0 bytes = not planned for this shape
        nb = lib.sar_conv2d_gemm_split_slab_bytes(C.byref(d))
        if nb > 0:
            kslab = kslab(nb // 4) if kslab is not None else torch.empty(nb // 4, dtype=torch.float32, device=src.device)
            assert kslab.dtype == torch.float32 and kslab.is_contiguous() and kslab.numel() >= nb // 4
            d.slab = ptr(kslab)
    if epi in (L.SAR_EPI_STATS, L.SAR_EPI_MASK):
        nparts = lib.sar_conv2d_gemm_split_nparts(C.byref(d)) if split else lib.sar_conv2d_nparts(C.byref(d))
        partials = _reducing_partials(d, nparts, "sar_conv2d_nparts", geo["M"], src.device)
    n_conv = geo["B"] * (geo["H_src"] * geo["W_src"] if geo.get("transposed") else geo["H_out"] * geo["W_out"])
    flops = 2.0 * geo["M"] * geo["Kc"] * geo["KH"] * geo["KW"] * n_conv
    tag = "conv2d_%dx%d%s" % (geo["KH"], geo["KW"], "_dgrad" if geo.get("transposed") else "")
    if split:
        mirror = "mirror" if (geo.get("transposed") and geo["stride"] == 1) else False
        (src_bound, w_bound), packed = _split_inputs(
            split, bounds, ((src, geo.get("pro")),), packed,
            lambda: _pack_split_conv2d(W, w_stride_tap, w_stride_c, geo["Kc"], geo["M"], split, mirror))
        with profiler.region(tag + "_split" + _shape_tag(geo), flops):
            check(lib.sar_conv2d_gemm_split(C.byref(d), L.SAR_SPLIT[split], ptr(packed), ptr(src_bound), ptr(w_bound), stream_ptr()),
                  "sar_conv2d_gemm_split")
    else:
        with profiler.region(tag + _shape_tag(geo), flops):
            check(lib.sar_conv2d_gemm_f32(C.byref(d), stream_ptr()), "sar_conv2d_gemm_f32")
    return (partials, nparts) if partials is not None else None


_C2D_WG_SLOTS = int(os.environ.get("SAR_C2D_WG_SLOTS", "512"))


def conv2d_wgrad(src, dout, dW_tcm, *, split="default", bounds=None, slabs=None, **geo):
    """dW in (tap, c, m) layout -> dW_tcm (flat, taps*Kc*M floats): sar_conv2d_wgrad_f32 -- or, with split="f16x3a" / "bf16x6" on 3x3 /
    stride 1 / pad 1 at image widths 8 / 16 / 32 / 64, sar_conv2d_wgrad_split (fp32 results on the fp16 / bf16 matrix pipe; bounds =
    (src_bound, dout_bound) cells, None = computed here by device kernels).  Slabs are summed in slab order either way."""
    lib = L.load()
    split = DEFAULT_SPLIT if split == "default" else split
    if split not in ("f16x3a", "bf16x6"):
        split = None
    d = _conv2d_desc(src, **geo)
    d.dout, d.ld_dout = ptr(_f32(dout)), dout.stride(0)
    taps = geo["KH"] * geo["KW"]
    n = taps * geo["Kc"] * geo["M"]
    flops = 2.0 * geo["M"] * geo["Kc"] * taps * geo["B"] * geo["H_out"] * geo["W_out"]
    if split:
        wk, kt = C.c_int(0), C.c_int(0)
        wgs = lib.sar_conv2d_wgrad_split_blocks(C.byref(d), L.SAR_SPLIT[split], C.byref(wk), C.byref(kt))
        if wgs == L.SAR_E_UNSUP:      # not built for this shape: the fp32 kernel
            split = None
        else:
            check(0 if wgs > 0 else (wgs or -1), "sar_conv2d_wgrad_split_blocks")
    if split:
        ntiles = (geo["B"] * geo["H_out"] * geo["W_out"] + kt.value - 1) // kt.value
        nsplit = max(1, min(ntiles, (_C2D_WG_SLOTS + wgs - 1) // wgs)) * wk.value      # one round of the resident workgroups (2 per CU)
    else:
        wgs = ((geo["M"] + 63) // 64) * max(1, (geo["Kc"] + 31) // 32)
        # one round of the 512 resident workgroups (2 per CU): measured 22 % faster than 768 / 1024 in isolation (the kernels do not
        # fit 3 per CU, so a larger grid runs a second, partly filled round)
        nsplit = max(1, min(geo["B"] * max(1, geo["H_out"] // 2), (_C2D_WG_SLOTS + wgs - 1) // wgs))
    slab = _wgrad_slab(d, slabs, dW_tcm, nsplit, n, src.device)
    if split:
        (sb, db), _ = _split_inputs(split, bounds, ((src, geo.get("pro")), (dout, None)))
        with profiler.region("conv2d_wgrad_3x3_split" + _shape_tag(geo), flops):
            check(lib.sar_conv2d_wgrad_split(C.byref(d), L.SAR_SPLIT[split], ptr(sb), ptr(db), stream_ptr()), "sar_conv2d_wgrad_split")
    else:
        with profiler.region("conv2d_wgrad_%dx%d" % (geo["KH"], geo["KW"]) + _shape_tag(geo), flops):
            check(lib.sar_conv2d_wgrad_f32(C.byref(d), stream_ptr()), "sar_conv2d_wgrad_f32")
    _wgrad_slab_done(slabs, slab, nsplit, n, dW_tcm)


def permute3(inp, out, d0, d1, d2, s0, s1, s2):
    check(L.load().sar_permute3_f32(ptr(inp), ptr(out), d0, d1, d2, s0, s1, s2, stream_ptr()), "sar_permute3_f32")


class PermuteBatch:
    """Many 3-d re-layouts between two flat fp32 buffers in ONE launch (sar_permute3_batch_f32)."""

    ITEM = [("src_off", "<i8"), ("dst_off", "<i8"), ("s0", "<i8"), ("s1", "<i8"), ("s2", "<i8"),
            ("d0", "<i4"), ("d1", "<i4"), ("d2", "<i4"), ("reserved", "<i4")]

    def __init__(self):
        self.items = []

    def add(self, src_off, dst_off, d0, d1, d2, s0, s1, s2):
        self.items.append((src_off, dst_off, s0, s1, s2, d0, d1, d2, 0))

    def finalize(self, device):
        import numpy as np
        tab = np.array(self.items, dtype=np.dtype(self.ITEM, align=True))
        assert tab.dtype.itemsize == 56          # sizeof(sar_permute_item)
        self.table = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(device)
        self.max_elems = max(it[5] * it[6] * it[7] for it in self.items)

    def run(self, src, dst):
        check(L.load().sar_permute3_batch_f32(ptr(_f32(src)), ptr(_f32(dst)), ptr(self.table), len(self.items), self.max_elems,
                                              stream_ptr()), "sar_permute3_batch_f32")


def bn_relu_maxpool_fwd(x, scale, shift, y, B, H, W):
    check(L.load().sar_bn_relu_maxpool_fwd_f32(ptr(x), ptr(scale), ptr(shift), ptr(y), x.shape[0], B, H, W, x.stride(0),
                                               y.stride(0), stream_ptr()), "sar_bn_relu_maxpool_fwd_f32")


def bn_relu_maxpool_bwd(x, scale, shift, mean, dy, dz, B, H, W):
    Cc = x.shape[0]
    nparts = L.load().sar_bn_relu_maxpool_bwd_nparts(B, H, W)
    partials = torch.empty((Cc, nparts, 2), dtype=torch.float32, device=x.device)
    check(L.load().sar_bn_relu_maxpool_bwd_f32(ptr(x), ptr(scale), ptr(shift), ptr(mean), ptr(dy), ptr(dz), ptr(partials),
                                               nparts, Cc, B, H, W, x.stride(0), dy.stride(0), stream_ptr()),
          "sar_bn_relu_maxpool_bwd_f32")
    return partials, nparts


def adam(w, m, v, g, lr_dev, step_dev, beta1=0.9, beta2=0.999, eps=1e-8):
    check(L.load().sar_adam_f32(ptr(w), ptr(m), ptr(v), ptr(g), w.numel(), ptr(lr_dev), ptr(step_dev), beta1, beta2, eps,
                                stream_ptr()), "sar_adam_f32")


def conv2d_stem_dgrad(dout, w_packed, dx, *, B, H, W, H_out, W_out, M, KH, KW, stride, pad):
    """Image gradient of the one-input-channel stem conv (dout CN [M][B*Ho*Wo], w_packed [KH*KW][1][M])."""
    check(L.load().sar_conv2d_stem_dgrad_f32(ptr(_f32(dout)), dout.stride(0), ptr(_f32(w_packed)), B, H, W, H_out, W_out, M,
                                             KH, KW, stride, pad, ptr(dx), stream_ptr()), "sar_conv2d_stem_dgrad_f32")
