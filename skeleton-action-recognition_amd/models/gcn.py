"""Layer-level drop-ins for the reference's models/gcn.py: `GraphConv`, `GraphConvTD` and `AdjGraphConv` as torch modules whose
arithmetic runs in libsar_hip.so (fp32).

  GraphConv(filters)                        forward(x (N,C,V),   A (N,V,V), training) -> (x (N,filters,V),   A)    models/gcn.py:22-36
  GraphConvTD(filters, kernel_size=3)       forward(x (B,C,T,V), A (K,V,V), training) -> (x (B,filters,T,V), A)    models/gcn.py:187-209
  AdjGraphConv(filters, adjacency_matrix)   forward(x (B,C,T,V), training)            ->  x (B,filters,T,V)        models/gcn.py:212-238

Parameters keep the Keras layouts and names (`kernel` (1, C, filters) / (1, 1, C, K * filters) with channel k * filters + m, `bias`;
AdjGraphConv also owns the trainable `adjacency_matrix`), are created on the first call as Keras' `build` does (or by
load_state_dict), and are initialised with VarianceScaling(2, fan_out, truncated_normal), biases zero, as sar_amd/stgcn.py does.
Inputs are contiguous float32 CUDA tensors in the reference's NCHW order; anything else raises ValueError before a launch.  Only
the default einsum string of each layer is implemented; any other raises ValueError.

Each layer is ONE torch.autograd.Function over sar_amd.ops:
  * the 1x1 convolution is sar_conv_gemm_f32 (TEMPORAL, taps = 1) with its weight / data gradients;
  * GraphConv contracts with the per-sample adjacency on csrc/graph_sample.hip (V <= 512);
  * GraphConvTD takes the fused gather-list kernel (sar_conv_gemm_f32 GRAPH with GraphTables, exactly as the engine feeds it) when A
    does not require a gradient, has 3 slices and at most 4 non-zeros per column and per row; any other A -- and AdjGraphConv
    always -- takes the 1x1 product plus csrc/graph_dense.hip (V <= 32, K <= 8), which also yields dA.

The layers convert NCHW <-> the kernels' CN layout ([C][B*T*V]) at their boundary with the permute kernel.  A network composed
of these layers pays that conversion PER LAYER; the whole-network engines (models/stgcn.py, stgin.py, stpgcn.py, stgcn_debug.py)
convert once.  This is the interface for variants that are not pre-built, not the fast path.

Not here: GraphIsoConv / GraphIsoConvTD (models/gcn.py:54-163) -- models/stgin.py covers that model as a whole.
"""
import math

import numpy as np
import torch

from sar_amd import _lib as L
from sar_amd import ops

GRAPH_CONV_EINSUM = "ncv,nvw->ncw"
GRAPH_CONV_TD_EINSUM = "nkctv,kvw->nctw"


def _require(x, ndim, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == ndim and x.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 CUDA tensor with %d dimensions" % (what, ndim))


def _require_einsum(einsum, default):
    if einsum != default:
        raise ValueError("einsum %r is not implemented (only %r is)" % (einsum, default))


def to_cn(x):
    """(N, C, ...) -> CN matrix [C][N * inner] (sar_permute3_f32)"""
    N, C = x.shape[:2]
    inner = x.numel() // (N * C)
    out = torch.empty((C, N * inner), dtype=torch.float32, device=x.device)
    ops.permute3(x, out, C, N, inner, inner, C * inner, 1)
    return out


def from_cn(m, shape):
    """CN matrix [C][N * inner] -> contiguous (N, C, ...) of `shape`"""
    N, C = shape[:2]
    inner = m.shape[1] // N
    out = torch.empty(shape, dtype=torch.float32, device=m.device)
    ops.permute3(m, out, N, C, inner, inner, N * inner, 1)
    return out


def variance_scaling_(kernel):
    """VarianceScaling(2, fan_out, truncated_normal) of a Keras kernel (.., in, out), as sar_amd/stgcn.py _init_params"""
    shp = tuple(kernel.shape)
    std = math.sqrt(2.0 / (int(np.prod(shp[:-2])) * shp[-1])) / .87962566103423978
    w = torch.empty(shp, dtype=torch.float64)
    torch.nn.init.trunc_normal_(w, 0.0, std, -2 * std, 2 * std)
    with torch.no_grad():
        kernel.copy_(w.to(torch.float32))


# ---- the 1x1 convolution shared by the three layers: columns (B, T, V) of a CN matrix, V <= 64 (sar_conv_gemm_f32's limit)
def _conv1x1_fwd(X, W, bias, geo):
    C, M = W.shape
    y = torch.empty((M, X.shape[1]), dtype=torch.float32, device=X.device)
    ops.conv_gemm(L.SAR_CONV_TEMPORAL, X, y, W, 0, M, Kc=C, M=M, taps=1, stride=1, pad=0, bias=bias, split=None, **geo)
    return y


def _conv1x1_bwd(X, dy, W, geo, need_w, need_dx):
    """(dW (C, M), dbias (M), dX), each None when not asked for: the weight and bias gradients are one launch, dX another"""
    C, M = W.shape
    dW = db = dX = None
    if need_w:
        flat = torch.empty(C * M + M, dtype=torch.float32, device=X.device)
        ops.conv_wgrad(L.SAR_CONV_TEMPORAL, X, dy, flat, Kc=C, M=M, taps=1, stride=1, pad=0, w_stride_tap=0, w_stride_c=M,
                       wsize=C * M, bsize=M, split=None, **geo)
        dW, db = flat[:C * M], flat[C * M:]
    if need_dx:
        WT = torch.empty((M, C), dtype=torch.float32, device=X.device)
        ops.transpose(W, WT, 1, C, M)
        dX = torch.empty((C, X.shape[1]), dtype=torch.float32, device=X.device)
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, dy, dX, WT, 0, C, Kc=M, M=C, taps=1, stride=1, pad=0, transposed=True, split=None, **geo)
    return dW, db, dX


def _column_geometry(N, V):
    """a (B, T, V') factorisation of the N * V columns with V' <= 64: the 1x1 product does not care which"""
    vf = max(d for d in range(1, min(V, 64) + 1) if V % d == 0)
    return dict(B=N, V=vf, T_src=V // vf, T_out=V // vf)


class _GraphConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, A, kernel, bias):
        N, C, V = x.shape
        F = bias.shape[0]
        geo = _column_geometry(N, V)
        X = to_cn(x)
        y = _conv1x1_fwd(X, kernel.view(C, F), bias, geo)
        out = torch.empty_like(y)
        ops.graph_sample_fwd(y, A, out, F, V, N)
        ctx.save_for_backward(X, y, A, kernel)
        ctx.geo, ctx.shape = geo, (N, C, V)
        return from_cn(out, (N, F, V))

    @staticmethod
    def backward(ctx, dout):
        X, y, A, kernel = ctx.saved_tensors
        N, C, V = ctx.shape
        F = kernel.shape[-1]
        need_x, need_A, need_k, need_b = ctx.needs_input_grad
        dc = to_cn(dout.contiguous())
        dA = dW = db = dX = None
        if need_A:
            dA = torch.empty_like(A)
            ops.graph_sample_dA(y, dc, dA, F, V, N)
        if need_x or need_k or need_b:       # (only A asks for a gradient: nothing below is launched)
            dy = torch.empty_like(dc)
            ops.graph_sample_bwd_data(dc, A, dy, F, V, N)
            dW, db, dX = _conv1x1_bwd(X, dy, kernel.view(C, F), ctx.geo, need_k or need_b, need_x)
        return (from_cn(dX, (N, C, V)) if dX is not None else None), dA, (dW.view(kernel.shape) if dW is not None else None), db


class _GraphConvTDDenseFn(torch.autograd.Function):
    """Conv2D(K F, 1x1) then the dense contraction with A (K, V, V): csrc/graph_dense.hip, dA included"""

    @staticmethod
    def forward(ctx, x, A, kernel, bias):
        B, C, T, V = x.shape
        K = A.shape[0]
        F = bias.shape[0] // K
        geo = dict(B=B, V=V, T_src=T, T_out=T)
        X = to_cn(x)
        y3 = _conv1x1_fwd(X, kernel.view(C, K * F), bias, geo)
        g = torch.empty((F, X.shape[1]), dtype=torch.float32, device=x.device)
        ops.graph_dense_fwd(y3, A, g, K, F, V, B * T)
        ctx.save_for_backward(X, y3, A, kernel)
        ctx.geo, ctx.shape = geo, (B, C, T, V)
        return from_cn(g, (B, F, T, V))

    @staticmethod
    def backward(ctx, dout):
        X, y3, A, kernel = ctx.saved_tensors
        B, C, T, V = ctx.shape
        K = A.shape[0]
        F = kernel.shape[-1] // K
        need_x, need_A, need_k, need_b = ctx.needs_input_grad
        dg = to_cn(dout.contiguous())
        dA = dW = db = dX = None
        if need_A:
            dA = torch.empty_like(A)
            ops.graph_dense_dA(y3, dg, dA, K, F, V, B * T)
        if need_x or need_k or need_b:
            dy3 = torch.empty_like(y3)
            ops.graph_dense_bwd_data(dg, A, dy3, K, F, V, B * T)
            dW, db, dX = _conv1x1_bwd(X, dy3, kernel.view(C, K * F), ctx.geo, need_k or need_b, need_x)
        return (from_cn(dX, (B, C, T, V)) if dX is not None else None), dA, (dW.view(kernel.shape) if dW is not None else None), db


class _GraphConvTDFusedFn(torch.autograd.Function):
    """the fixed sparse adjacency folded into the operand load as <= 4-entry gather lists (sar_conv_gemm_f32 GRAPH), the call the
    engine's block makes; the 3 F-channel tensor is never materialised"""

    @staticmethod
    def forward(ctx, x, tables, kernel, bias):
        B, C, T, V = x.shape
        tab_fwd, tab_bwd = tables
        K = tab_fwd.K
        F = bias.shape[0] // K
        geo = dict(B=B, V=V, T_src=T, T_out=T)
        X = to_cn(x)
        g = torch.empty((F, X.shape[1]), dtype=torch.float32, device=x.device)
        ops.conv_gemm(L.SAR_CONV_GRAPH, X, g, kernel.view(C, K * F), F, K * F, Kc=C, M=F, taps=K, bias=bias, tables=tab_fwd,
                      split=None, **geo)
        ctx.save_for_backward(X, kernel)
        ctx.geo, ctx.shape, ctx.tables = geo, (B, C, T, V), tables
        return from_cn(g, (B, F, T, V))

    @staticmethod
    def backward(ctx, dout):
        X, kernel = ctx.saved_tensors
        B, C, T, V = ctx.shape
        tab_fwd, tab_bwd = ctx.tables
        K = tab_fwd.K
        F = kernel.shape[-1] // K
        dg = to_cn(dout.contiguous())
        dW = db = dx = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            flat = torch.empty(C * K * F + K * F, dtype=torch.float32, device=X.device)
            ops.conv_wgrad(L.SAR_CONV_GRAPH, X, dg, flat, Kc=C, M=F, taps=K, tables=tab_fwd, w_stride_tap=F, w_stride_c=K * F,
                           wsize=C * K * F, bsize=K * F, split=None, **ctx.geo)
            dW, db = flat[:C * K * F].view(kernel.shape), flat[C * K * F:]
        if ctx.needs_input_grad[0]:
            gT = torch.empty((K, F, C), dtype=torch.float32, device=X.device)      # [k][f][c] = kernel[c][k F + f]
            ops.permute3(kernel, gT, K, F, C, F, 1, K * F)
            dX = torch.empty((C, X.shape[1]), dtype=torch.float32, device=X.device)
            ops.conv_gemm(L.SAR_CONV_GRAPH, dg, dX, gT, F * C, C, Kc=F, M=C, taps=K, tables=tab_bwd, split=None, **ctx.geo)
            dx = from_cn(dX, (B, C, T, V))
        return dx, None, dW, db


class _Conv1x1Layer(torch.nn.Module):
    """`kernel` / `bias` in the Keras layout, created on the first call (or by load_state_dict)"""

    def __init__(self, out_channels, kernel_rank):
        super().__init__()
        self.out_channels, self._kernel_rank = int(out_channels), kernel_rank
        self.register_parameter("kernel", None)
        self.register_parameter("bias", None)

    def build(self, in_channels, device):
        if self.kernel is None:
            shape = (1,) * (self._kernel_rank - 2) + (int(in_channels), self.out_channels)
            self.kernel = torch.nn.Parameter(torch.empty(shape, dtype=torch.float32, device=device))
            self.bias = torch.nn.Parameter(torch.zeros(self.out_channels, dtype=torch.float32, device=device))
            variance_scaling_(self.kernel)
        elif self.kernel.shape[-2] != in_channels:
            raise ValueError("the layer was built for %d input channels, got %d" % (self.kernel.shape[-2], in_channels))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if self.kernel is None and k is not None:
            self.build(k.shape[-2], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class GraphConv(_Conv1x1Layer):
    """models/gcn.py:22-36: Conv1D(filters, 1), then einsum 'ncv,nvw->ncw' with a per-sample adjacency"""

    def __init__(self, filters, einsum=GRAPH_CONV_EINSUM):
        _require_einsum(einsum, GRAPH_CONV_EINSUM)
        super().__init__(filters, 3)
        self.einsum = einsum

    def forward(self, x, A, training=None):
        _require(x, 3, "x (N, C, V)")
        _require(A, 3, "A (N, V, V)")
        N, C, V = x.shape
        if tuple(A.shape) != (N, V, V) or V > 512:
            raise ValueError("A must be (N, V, V) = (%d, %d, %d) with V <= 512, got %s" % (N, V, V, tuple(A.shape)))
        if N * V >= 1 << 22:
            raise ValueError("N * V = %d columns: the 1x1 product is built for fewer than 2^22" % (N * V))
        self.build(C, x.device)
        return _GraphConvFn.apply(x, A, self.kernel, self.bias), A


def _dense_limits(K, V):
    if V > 32 or K > 8:
        raise ValueError("the dense adjacency contraction is built for V <= 32 and K <= 8 (got V = %d, K = %d)" % (V, K))


class GraphConvTD(_Conv1x1Layer):
    """models/gcn.py:187-209: Conv2D(kernel_size * filters, 1x1), then einsum 'nkctv,kvw->nctw'"""

    def __init__(self, filters, kernel_size=3, einsum=GRAPH_CONV_TD_EINSUM):
        _require_einsum(einsum, GRAPH_CONV_TD_EINSUM)
        super().__init__(filters * kernel_size, 4)
        self.filters, self.kernel_size, self.einsum = int(filters), int(kernel_size), einsum
        self._tables_for, self._tables_key, self._tables = None, None, None

    def _gather_tables(self, A):
        """(forward, backward) GraphTables of a fixed A with <= 4 non-zeros per column and per row, else None; cached on the tensor's
        identity and version, so an A edited in place is re-tabled"""
        key = (A.data_ptr(), A._version)
        if self._tables_for is not A or key != self._tables_key:      # (the tensor is kept: its address cannot pass to another)
            self._tables_for = A
            host = A.detach().cpu().numpy()
            try:
                tables = (ops.GraphTables(host, A.device, transpose=False), ops.GraphTables(host, A.device, transpose=True))
            except ValueError:          # denser than the gather lists hold
                tables = None
            self._tables_key, self._tables = key, tables
        return self._tables

    def forward(self, x, A, training=None):
        _require(x, 4, "x (B, C, T, V)")
        _require(A, 3, "A (K, V, V)")
        B, C, T, V = x.shape
        K = self.kernel_size
        if tuple(A.shape) != (K, V, V) or V > 64:
            raise ValueError("A must be (K, V, V) = (%d, %d, %d) with V <= 64, got %s" % (K, V, V, tuple(A.shape)))
        if B * T * V >= 1 << 22:
            raise ValueError("B * T * V = %d columns: the convolutions are built for fewer than 2^22" % (B * T * V))
        tables = self._gather_tables(A) if (K == 3 and not A.requires_grad) else None
        if tables is None:
            _dense_limits(K, V)
        self.build(C, x.device)
        if tables is not None:
            return _GraphConvTDFusedFn.apply(x, tables, self.kernel, self.bias), A
        return _GraphConvTDDenseFn.apply(x, A, self.kernel, self.bias), A


class AdjGraphConv(_Conv1x1Layer):
    """models/gcn.py:212-238: GraphConvTD whose adjacency is the layer's own trainable variable `adjacency_matrix`"""

    def __init__(self, filters, adjacency_matrix, einsum=GRAPH_CONV_TD_EINSUM):
        _require_einsum(einsum, GRAPH_CONV_TD_EINSUM)
        A = torch.as_tensor(np.asarray(adjacency_matrix.detach().cpu() if isinstance(adjacency_matrix, torch.Tensor)
                                       else adjacency_matrix), dtype=torch.float32)
        if A.dim() != 3 or A.shape[1] != A.shape[2]:
            raise ValueError("adjacency_matrix must be (K, V, V), got %s" % (tuple(A.shape),))
        _dense_limits(A.shape[0], A.shape[1])
        super().__init__(filters * A.shape[0], 4)
        self.filters, self.kernel_size, self.einsum = int(filters), int(A.shape[0]), einsum
        self.adjacency_matrix = torch.nn.Parameter(A.contiguous().cuda())

    def forward(self, x, training=None):
        _require(x, 4, "x (B, C, T, V)")
        if x.shape[3] != self.adjacency_matrix.shape[1]:
            raise ValueError("x has %d joints, adjacency_matrix %d" % (x.shape[3], self.adjacency_matrix.shape[1]))
        self.build(x.shape[1], x.device)
        return _GraphConvTDDenseFn.apply(x, self.adjacency_matrix, self.kernel, self.bias)
