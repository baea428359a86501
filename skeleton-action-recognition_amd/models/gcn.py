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

Each layer call is ONE torch.autograd.Function over sar_amd.ops:
  * the 1x1 convolution is sar_conv_gemm_f32 (TEMPORAL, taps = 1) with its weight / data gradients, written once for every layer
    of this package and every layer wrapper: ops.conv1x1_fwd / conv1x1_wgrad / conv1x1_dgrad over ops.column_geometry;
  * _ConvContractFn is the 1x1 product followed by a contraction with A, parameterised by the contraction's three kernels:
    GraphConv contracts with the per-sample adjacency on csrc/graph_sample.hip (V <= 512);
  * GraphConvTD takes the fused gather-list kernel (_GraphConvTDFusedFn: sar_conv_gemm_f32 GRAPH with GraphTables, exactly as the
    engine feeds it; no intermediate) when A does not require a gradient, has 3 slices and at most 4 non-zeros per column and per
    row; any other A -- and AdjGraphConv always -- takes _ConvContractFn with csrc/graph_dense.hip (V <= 32, K <= 8), which also
    yields dA.
Every layer's `kernel` / `bias` (and a GIN MLP layer's BatchNorm) live in one lazily built class, _Conv1x1Layer.

The layers convert NCHW <-> the kernels' CN layout ([C][B*T*V]) at their boundary with the permute kernel.  A network composed
of these layers pays that conversion PER LAYER; the whole-network engines (models/stgcn.py, stgin.py, stpgcn.py, stgcn_debug.py)
convert once.  This is the interface for variants that are not pre-built, not the fast path.

The graph isomorphism layers (models/gcn.py:54-163; `filters` is the list of MLP widths, activation 'relu' only):

  GraphIsoConv(filters, return_logits=False)        forward(x (N,C,V),   A (N,V,V),   training) -> (x (N,filters[-1],V),   A)    models/gcn.py:54-93
  GraphIsoConvTD(filters, kernel_size=3)            forward(x (B,C,T,V), A (K-1,V,V), training) -> (x (B,filters[-1],T,V), A)    models/gcn.py:112-163

Both own the trainable scalar `epsilon` and the MLP(s) `mlp.{i}.*` / `mlps.{k}.{i}.*` (kernel, bias, gamma, beta; moving_mean and
moving_var as buffers; BatchNorm eps 1e-3, momentum 0.99); see the classes.  training=False uses the moving statistics and is
forward only.  The MLP arithmetic is written once, for K branches stacked along the channel axis (_mlp_forward / _mlp_backward):
GraphIsoConv is its K = 1 case behind the per-sample aggregation, GraphIsoConvTD its K = kernel_size case behind the table
expansion; the two autograd Functions hold only what is in front of the MLP and its gradient.
"""
import collections
import math

import numpy as np
import torch

from sar_amd import _lib as L
from sar_amd import ops

GRAPH_CONV_EINSUM = "ncv,nvw->ncw"
GRAPH_CONV_TD_EINSUM = "nkctv,kvw->nctw"
GRAPH_ISO_CONV_TD_EINSUM = "nctv,kvw->nkctw"
BN_EPS, BN_MOMENTUM = 1e-3, 0.99          # Keras BatchNormalization defaults, as sar_amd/stgcn.py


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


# (forward, data gradient, adjacency gradient) of the two contractions behind a 1x1 product, each called as op(in, A, out, *dims)
# (the adjacency gradient as op(y, dout, dA, *dims))
SAMPLE_CONTRACTION = (ops.graph_sample_fwd, ops.graph_sample_bwd_data, ops.graph_sample_dA)      # dims (F, V, N): A (N, V, V), V <= 512
DENSE_CONTRACTION = (ops.graph_dense_fwd, ops.graph_dense_bwd_data, ops.graph_dense_dA)          # dims (K, F, V, B T): A (K, V, V)


class _ConvContractFn(torch.autograd.Function):
    """the 1x1 convolution, then `contraction` with A: GraphConv (SAMPLE_CONTRACTION), the dense path of GraphConvTD and AdjGraphConv
    (DENSE_CONTRACTION, dA included).  F = the channels that leave the contraction, geo = the column geometry of the product,
    columns = (NCHW -> CN, CN -> NCHW of a given shape): a layer whose contraction wants another column order brings its own pair"""

    @staticmethod
    def forward(ctx, x, A, kernel, bias, contraction, dims, F, geo, columns=(to_cn, from_cn)):
        C = x.shape[1]
        to_cn, from_cn = columns
        X = to_cn(x)
        y = ops.conv1x1_fwd(X, kernel.view(C, -1), bias, geo)
        out = torch.empty((F, X.shape[1]), dtype=torch.float32, device=x.device)
        contraction[0](y, A, out, *dims)
        ctx.save_for_backward(X, y, A, kernel)
        ctx.contraction, ctx.dims, ctx.geo, ctx.shape, ctx.columns = contraction, dims, geo, tuple(x.shape), columns
        return from_cn(out, (x.shape[0], F) + tuple(x.shape[2:]))

    @staticmethod
    def backward(ctx, dout):
        X, y, A, kernel = ctx.saved_tensors
        _, bwd_data, adjacency_grad = ctx.contraction
        to_cn, from_cn = ctx.columns
        C = ctx.shape[1]
        need_x, need_A, need_k, need_b = ctx.needs_input_grad[:4]
        dc = to_cn(dout.contiguous())
        dA = dW = db = dx = None
        if need_A:
            dA = torch.empty_like(A)
            adjacency_grad(y, dc, dA, *ctx.dims)
        if need_x or need_k or need_b:       # (only A asks for a gradient: nothing below is launched)
            dy = torch.empty_like(y)
            bwd_data(dc, A, dy, *ctx.dims)
            W = kernel.view(C, -1)
            if need_k or need_b:
                dW, db = ops.conv1x1_wgrad(X, dy, ctx.geo)
                dW = dW.view(kernel.shape)
            if need_x:
                dx = from_cn(ops.conv1x1_dgrad(dy, W, ctx.geo), ctx.shape)
        return dx, dA, dW, db, None, None, None, None, None


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
    """Conv(out_channels, 1x1) [-> BatchNormalization(axis=1), has_bn]: `kernel` / `bias` in the Keras layout, with a BatchNorm also
    `gamma` / `beta` and the buffers `moving_mean` / `moving_var`; created on the first call (or by load_state_dict)"""

    def __init__(self, out_channels, kernel_rank, has_bn=False):
        super().__init__()
        self.out_channels, self._kernel_rank, self.has_bn = int(out_channels), kernel_rank, bool(has_bn)
        self.register_parameter("kernel", None)
        self.register_parameter("bias", None)
        if self.has_bn:
            self.register_parameter("gamma", None)
            self.register_parameter("beta", None)
            self.register_buffer("moving_mean", None)
            self.register_buffer("moving_var", None)

    def build(self, in_channels, device):
        if self.kernel is None:
            f = self.out_channels
            new = lambda fill: torch.full((f,), fill, dtype=torch.float32, device=device)
            shape = (1,) * (self._kernel_rank - 2) + (int(in_channels), f)
            self.kernel = torch.nn.Parameter(torch.empty(shape, dtype=torch.float32, device=device))
            variance_scaling_(self.kernel)
            self.bias = torch.nn.Parameter(new(0.0))
            if self.has_bn:
                self.gamma, self.beta = torch.nn.Parameter(new(1.0)), torch.nn.Parameter(new(0.0))
                self.moving_mean, self.moving_var = new(0.0), new(1.0)
        elif self.kernel.shape[-2] != in_channels:
            raise ValueError("the layer was built for %d input channels, got %d" % (self.kernel.shape[-2], in_channels))

    def tensors(self):
        return [self.kernel, self.bias] + ([self.gamma, self.beta] if self.has_bn else [])

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
        return _ConvContractFn.apply(x, A, self.kernel, self.bias, SAMPLE_CONTRACTION, (self.out_channels, V, N), self.out_channels,
                                     ops.column_geometry(N, V)), A


def _dense_limits(K, V):
    if V > 32 or K > 8:
        raise ValueError("the dense adjacency contraction is built for V <= 32 and K <= 8 (got V = %d, K = %d)" % (V, K))


def _conv_then_dense(layer, x, A):
    """Conv2D(K F, 1x1) of `layer`, then the dense contraction with A (K, V, V): csrc/graph_dense.hip, dA included"""
    B, C, T, V = x.shape
    K, F = layer.kernel_size, layer.filters
    return _ConvContractFn.apply(x, A, layer.kernel, layer.bias, DENSE_CONTRACTION, (K, F, V, B * T), F, dict(B=B, V=V, T_src=T, T_out=T))


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
        return _conv_then_dense(self, x, A), A


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
        return _conv_then_dense(self, x, self.adjacency_matrix)


# ================================================================================================ graph isomorphism layers
class _BNState:
    """what one BatchNorm of one call leaves for its consumers and for backward (fresh per call: nothing is shared between calls)"""

    def __init__(self, C, device):
        z = lambda: torch.empty(C, dtype=torch.float32, device=device)
        self.mean, self.rstd, self.scale, self.shift = z(), z(), z(), z()
        self.k1, self.k2, self.k3 = z(), z(), z()


def _rows(t, k, h):
    """rows k h .. (k + 1) h of a stacked tensor; a single branch's rows are the tensor itself (no view is made)"""
    return t if h == t.shape[0] else t[k * h:(k + 1) * h]


def _check_gin_arguments(filters, activation, return_logits, einsum, default_einsum):
    if activation != "relu":
        raise ValueError("activation %r is not implemented (only 'relu' is)" % (activation,))
    _require_einsum(einsum, default_einsum)
    if not isinstance(filters, list) or not filters or not all(isinstance(f, int) and f > 0 for f in filters):
        raise ValueError("filters must be a non-empty list of positive ints, got %r" % (filters,))


def _mlp(filters, kernel_rank, return_logits):
    last = len(filters) - 1
    return torch.nn.ModuleList(_Conv1x1Layer(f, kernel_rank, i < last or not return_logits) for i, f in enumerate(filters))


def _bn_forward(st, k, result, count, layer, training, unbiased):
    """BatchNorm of `layer` into branch k's rows of the stacked state `st`: training, from the producer's statistics (moving
    statistics updated); inference, from the moving statistics"""
    view = lambda t: _rows(t, k, layer.out_channels)
    if training:
        ops.bn_finalize(result[0], result[1], layer.out_channels, count, BN_EPS, BN_MOMENTUM, unbiased, layer.gamma, layer.beta,
                        layer.moving_mean, layer.moving_var, view(st.mean), view(st.rstd), view(st.scale), view(st.shift))
    else:
        ops.bn_eval_affine(layer.gamma, layer.beta, layer.moving_mean, layer.moving_var, BN_EPS, view(st.scale), view(st.shift))


def _bn_backward(st, k, sums, count, f, gamma):
    """(dgamma, dbeta) of the f-channel BatchNorm in branch k's rows of `st` and k1..k3 of its backward apply pass, from
    (partials (f, nparts, 2), nparts) = (sum dz, sum dz (a - mean)) per channel and partial"""
    view = lambda t: _rows(t, k, f)
    dg = torch.empty(2 * f, dtype=torch.float32, device=gamma.device)
    ops.bn_bwd_finalize(sums[0], sums[1], sums[1] * 2, 2, 0, 1, f, count, gamma, view(st.mean), view(st.rstd), dg[:f], dg[f:],
                        view(st.k1), view(st.k2), view(st.k3))
    return dg[:f], dg[f:]


_MLPSaved = collections.namedtuple("_MLPSaved", "K geo n src acts states")      # one call's state between _mlp_forward and _mlp_backward


def _mlp_forward(src, branches, geo, n, training, unbiased):
    """The K = len(branches) GIN MLPs, stacked along the channel axis: branch k (a chain of _Conv1x1Layer, all chains of one shape)
    reads rows k of src [K cin][n].  Every layer is the 1x1 product with the statistics epilogue (training), its BN + ReLU folded
    into the next product's operand load; the last BN + ReLU and the sum over the branches are sar_gin_sum_fwd_f32.  The
    element-wise passes are one launch for all branches; the BatchNorm finalisations run per branch on each layer's own gamma /
    beta / moving statistics (`unbiased`: the moving variance's convention).  A last layer without a BatchNorm (return_logits) is
    returned as it is, which a sum over branches cannot be.  -> (out [f_last][n], what _mlp_backward needs)"""
    K, dev = len(branches), src.device
    assert K == 1 or branches[0][-1].has_bn
    new = lambda rows: torch.empty((rows, n), dtype=torch.float32, device=dev)
    saved = _MLPSaved(K, geo, n, src, [], [])
    cin, prev = src.shape[0] // K, None
    for i, first in enumerate(branches[0]):
        f, stats = first.out_channels, first.has_bn and training
        a, st = new(K * f), _BNState(K * f, dev) if first.has_bn else None
        if stats:
            nparts = ops.conv_gemm_nparts(Kc=cin, M=f, **geo)
            part = torch.empty((K * f, nparts, 2), dtype=torch.float32, device=dev)
        for k, chain in enumerate(branches):
            l = chain[i]
            kw = dict(pro=(_rows(prev.scale, k, cin), _rows(prev.shift, k, cin)), pro_relu=True) if prev is not None else {}
            if stats:
                kw.update(epi=L.SAR_EPI_STATS, partials_out=_rows(part, k, f))
            ops.conv1x1_fwd(_rows(src, k, cin), l.kernel.view(cin, f), l.bias, geo, out=_rows(a, k, f), **kw)
            if l.has_bn:
                _bn_forward(st, k, (_rows(part, k, f), nparts) if stats else None, n, l, training, unbiased)
        saved.acts.append(a), saved.states.append(st)
        src, cin, prev = a, f, st
    out = src
    if prev is not None:
        out = new(cin)
        ops.gin_sum_fwd(src, prev.scale, prev.shift, K, out)
    return out, saved


def _mlp_backward(saved, params, da):
    """Backward of _mlp_forward (training): `params` = what the layers' tensors() gave, branch by branch and layer by layer, as
    autograd saved them; da = the gradient of `out` (CN).  -> (the gradient of the stacked source, the gradients in the order of
    `params`).  Layer i of branch k owns the slots 4 (k depth + i) .. + 3 = kernel, bias, gamma, beta: only the last layer of a
    single branch may lack the last two, and nothing follows it."""
    K, geo, n, src0, acts, states = saved
    depth, dev = len(acts), da.device
    new = lambda rows: torch.empty((rows, n), dtype=torch.float32, device=dev)
    at = lambda k, i: 4 * (k * depth + i)
    grads = [None] * len(params)
    st, a = states[-1], acts[-1]
    if st is not None:                        # the last BN + ReLU (and the sum over the branches)
        f = a.shape[0] // K
        sums = ops.gin_bwd_reduce(da, a, st.scale, st.shift, st.mean, K)
        for k in range(K):
            j = at(k, depth - 1)
            grads[j + 2], grads[j + 3] = _bn_backward(st, k, (_rows(sums[0], k, f), sums[1]), n, f, params[j + 2])
        dz = new(K * f)
        ops.gin_bwd_apply(da, a, st.scale, st.shift, (st.k1, st.k2, st.k3), K, dz)
        da = dz
    for i in range(depth - 1, -1, -1):
        f = acts[i].shape[0] // K
        src, pst = (acts[i - 1], states[i - 1]) if i else (src0, None)
        cin = src.shape[0] // K
        dsrc = new(K * cin)
        if i:
            npm = ops.conv_gemm_nparts(Kc=f, M=cin, transposed=True, epi=L.SAR_EPI_MASK, **geo)
            pm = torch.empty((K * cin, npm, 2), dtype=torch.float32, device=dev)
        for k in range(K):
            j, s_k, da_k = at(k, i), _rows(src, k, cin), _rows(da, k, f)
            pro = (_rows(pst.scale, k, cin), _rows(pst.shift, k, cin)) if i else None
            dW, grads[j + 1] = ops.conv1x1_wgrad(s_k, da_k, geo, pro=pro, pro_relu=pro is not None)
            grads[j] = dW.view(params[j].shape)
            # through the hidden BN + ReLU: masked data gradient + BatchNorm-backward sums
            mask = dict(epi=L.SAR_EPI_MASK, aux=s_k, aux_affine=pro, aux_mean=_rows(pst.mean, k, cin),
                        partials_out=_rows(pm, k, cin)) if i else {}
            ops.conv1x1_dgrad(da_k, params[j].view(cin, f), geo, out=_rows(dsrc, k, cin), **mask)
            if i:
                jp = at(k, i - 1)
                grads[jp + 2], grads[jp + 3] = _bn_backward(pst, k, (_rows(pm, k, cin), npm), n, cin, params[jp + 2])
        if i:
            ops.affine2(dsrc, src, (pst.k1, pst.k2, pst.k3), dsrc)
        da = dsrc
    return da, grads


class _GraphIsoConvFn(torch.autograd.Function):
    """GraphIsoConv as one node: the fused aggregation (csrc/graph_sample.hip, SELF), then the MLP as _mlp_forward's single branch
    (rows = the whole tensor).  Everything backward needs is kept in ctx."""

    @staticmethod
    def forward(ctx, x, A, layer, training, eps, *params):
        N, C, V = x.shape
        X = to_cn(x)
        agg = torch.empty_like(X)
        ops.gin_sample_fwd(X, A, eps, agg, C, V, N)
        # Keras' non-fused 3-D path: biased moving variance
        out, ctx.mlp = _mlp_forward(agg, layer._all_layers(), ops.column_geometry(N, V), N * V, training, False)
        ctx.save_for_backward(A, eps, *params)
        ctx.training, ctx.X = training, X
        return from_cn(out, (N, out.shape[0], V))

    @staticmethod
    def backward(ctx, dout):
        if not ctx.training:
            raise RuntimeError("backward through GraphIsoConv(x, A, training=False) is not supported (inference path)")
        A, eps = ctx.saved_tensors[:2]
        C, (N, V) = ctx.X.shape[0], A.shape[:2]
        da, grads = _mlp_backward(ctx.mlp, ctx.saved_tensors[2:], to_cn(dout.contiguous()))
        need_x, need_A, _, _, need_eps = ctx.needs_input_grad[:5]
        dx = dA = deps = None
        if need_eps:
            deps = torch.empty((), dtype=torch.float32, device=da.device)
            ops.gin_sample_eps_grad(ctx.X, da, deps, C, V, N)
        if need_A:
            dA = torch.empty_like(A)
            ops.graph_sample_dA(ctx.X, da, dA, C, V, N)
        if need_x:
            dX = torch.empty_like(ctx.X)
            ops.gin_sample_bwd_data(da, A, eps, dX, C, V, N)
            dx = from_cn(dX, (N, C, V))
        return (dx, dA, None, None, deps) + tuple(grads)


class _GinBase(torch.nn.Module):
    """`epsilon` and the MLP chains of _all_layers() (a subclass's), created on the first call or by load_state_dict, which finds the
    input width in the state dict's entry _first_kernel (a subclass's)"""

    def build(self, in_channels, device):
        layers = self._all_layers()
        if self.epsilon is None:
            self.epsilon = torch.nn.Parameter(torch.zeros((), dtype=torch.float32, device=device))
            for chain in layers:
                cin = int(in_channels)
                for l in chain:
                    l.build(cin, device)
                    cin = l.out_channels
        elif layers[0][0].kernel.shape[-2] != in_channels:
            raise ValueError("the layer was built for %d input channels, got %d" % (layers[0][0].kernel.shape[-2], in_channels))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + self._first_kernel)
        if self.epsilon is None and k is not None:
            self.build(k.shape[-2], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _call(self, fn, x, A, training):
        self.build(x.shape[1], x.device)
        params = [t for chain in self._all_layers() for l in chain for t in l.tensors()]
        return fn.apply(x, A, self, bool(self.training if training is None else training), self.epsilon, *params), A


class GraphIsoConv(_GinBase):
    """models/gcn.py:54-93: x = einsum('ncv,nvw->ncw', x, A + diag(1 + epsilon)); x = mlp(x), the MLP a chain of
    Conv1D(f, 1) -> BatchNormalization(axis=1) -> ReLU over `filters` (return_logits=True: the last layer is the bare Conv1D).
    Parameters: `epsilon` (), `mlp.{i}.kernel` (1, Cin, f), `mlp.{i}.bias`, `mlp.{i}.gamma` / `.beta` and the buffers
    `mlp.{i}.moving_mean` / `.moving_var` where layer i has a BatchNorm.  The statistics run over (N, V); the moving variance takes
    the BIASED batch variance (Keras' non-fused path for 3-D inputs; SURVEY 8(c), the data_bn convention).
    A + diag(..) is never formed (csrc/graph_sample.hip).  V <= 512, N V < 2^22.  A that requires a gradient gets dA."""

    def __init__(self, filters, activation="relu", return_logits=False, einsum=GRAPH_CONV_EINSUM):
        super().__init__()
        _check_gin_arguments(filters, activation, return_logits, einsum, GRAPH_CONV_EINSUM)
        self.filters, self.return_logits, self.einsum = list(filters), bool(return_logits), einsum
        self.mlp = _mlp(self.filters, 3, self.return_logits)
        self.register_parameter("epsilon", None)

    _first_kernel = "mlp.0.kernel"

    def _all_layers(self):
        return [list(self.mlp)]

    def forward(self, x, A, training=None):
        _require(x, 3, "x (N, C, V)")
        _require(A, 3, "A (N, V, V)")
        N, C, V = x.shape
        if tuple(A.shape) != (N, V, V) or V > 512:
            raise ValueError("A must be (N, V, V) = (%d, %d, %d) with V <= 512, got %s" % (N, V, V, tuple(A.shape)))
        if N * V >= 1 << 22:
            raise ValueError("N * V = %d columns: the 1x1 products are built for fewer than 2^22" % (N * V))
        return self._call(_GraphIsoConvFn, x, A, training)


class _GraphIsoConvTDFn(torch.autograd.Function):
    """GraphIsoConvTD as one node, composed from the kernels sar_amd/stgin.py runs for a dense adjacency: the table
    [A_k^T.., (1 + eps) I] (sar_gin_adjacency_f32), x expanded to the K slices (sar_graph_dense_bwd_data_f32), then the K MLPs as
    _mlp_forward's stacked branches.  Backward: the table's gradient (sar_graph_dense_dadj_f32 on (dz, x)) gives dA as its transpose
    and d epsilon as the trace of its self slice, which sar_gin_eps_grad_bn_f32 then replaces by the well-conditioned closed form.
    Everything backward needs is kept in ctx."""

    @staticmethod
    def forward(ctx, x, A, layer, training, eps, *params):
        B, C, T, V = x.shape
        K, n, dev = layer.kernel_size, B * T * V, x.device
        X = to_cn(x)
        table = torch.empty((K, V, V), dtype=torch.float32, device=dev)
        escale = torch.empty(C, dtype=torch.float32, device=dev)
        ops.gin_adjacency(A, eps, table, escale)
        z = torch.empty((K * C, n), dtype=torch.float32, device=dev)      # z[k C + c] = x[c] . A_k, the self slice (1 + eps) x[c]
        ops.graph_dense_bwd_data(X, table, z, K, C, V, B * T)
        # the fused 4-D convention of the engines: unbiased moving variance
        out, ctx.mlp = _mlp_forward(z, layer._all_layers(), dict(B=B, V=V, T_src=T, T_out=T), n, training, True)
        ctx.save_for_backward(A, eps, *params)
        ctx.training, ctx.shape, ctx.X, ctx.table = training, (B, C, T, V), X, table
        return from_cn(out, (B, out.shape[0], T, V))

    @staticmethod
    def backward(ctx, dout):
        if not ctx.training:
            raise RuntimeError("backward through GraphIsoConvTD(x, A, training=False) is not supported (inference path)")
        A, eps = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        (B, C, T, V), K, dev = ctx.shape, ctx.table.shape[0], dout.device
        da, grads = _mlp_backward(ctx.mlp, params, to_cn(dout.contiguous()))
        need_x, need_A, _, _, need_eps = ctx.needs_input_grad[:5]
        dx = dA = deps = None
        if need_A or need_eps:                 # the table's gradient: dA[k] is its transpose, d epsilon the trace of its self slice
            dtable = torch.empty((K, V, V), dtype=torch.float32, device=dev)
            ops.graph_dense_dA(da, ctx.X, dtable, K, C, V, B * T)
            if need_A:
                dA = torch.empty_like(A)
                if K > 1:
                    ops.transpose(dtable, dA, K - 1, V, V)
            if need_eps:                       # trace = <dtable[K - 1], I> (sar_gin_eps_grad_f32 also rescales its first operand:
                deps = torch.empty((), dtype=torch.float32, device=dev)      # dtable is not read again)
                eye = torch.eye(V, dtype=torch.float32, device=dev)
                ops.gin_eps_grad(dtable[K - 1], eye, eps, deps)
                # ... which fp32 leaves 1e-3 .. 1e-1 off: the self slice feeds Conv -> BatchNorm, whose output does not depend on the
                # scale 1 + eps of its input but for BN_EPS, so d epsilon is what is left of terms that cancel to ~1e-3.  The closed
                # form from that BatchNorm's backward (csrc/gin.hip) replaces the trace unless 1 + eps == 0
                j0 = 4 * (K - 1) * len(ctx.mlp.acts)                 # the self branch's first layer: kernel, bias, gamma, beta
                gamma = params[j0 + 2]
                ops.gin_eps_grad_bn(gamma, grads[j0 + 2], _rows(ctx.mlp.states[0].rstd, K - 1, gamma.numel()), BN_EPS, eps, deps)
        if need_x:
            dX = torch.empty_like(ctx.X)
            ops.graph_dense_fwd(da, ctx.table, dX, K, C, V, B * T)
            dx = from_cn(dX, (B, C, T, V))
        return (dx, dA, None, None, deps) + tuple(grads)


class GraphIsoConvTD(_GinBase):
    """models/gcn.py:112-163: x' = einsum('nctv,kvw->nkctw', x, concat(A, diag(1 + epsilon))); slice k through its own MLP
    (Conv2D(f, 1x1) -> BatchNormalization(axis=1) -> ReLU over `filters`); sum over the slices.  A is (kernel_size - 1, V, V).
    Parameters: `epsilon` (), `mlps.{k}.{i}.kernel` (1, 1, Cin, f), `.bias`, `.gamma`, `.beta` and the buffers `.moving_mean` /
    `.moving_var` (statistics over (B, T, V); unbiased moving variance, the fused 4-D convention of the engines).
    V <= 32, kernel_size <= 8, B T V < 2^22.  A that requires a gradient gets dA.
    Not built: return_logits=True (there is no branch sum without the ReLU) raises ValueError; there is no gather-list fast path for a
    fixed sparse A here -- every A takes the dense contraction (csrc/graph_dense.hip); models/stgin.py stays the fast path for the
    fixed graph."""

    def __init__(self, filters, kernel_size=3, activation="relu", return_logits=False, einsum=GRAPH_ISO_CONV_TD_EINSUM):
        super().__init__()
        _check_gin_arguments(filters, activation, return_logits, einsum, GRAPH_ISO_CONV_TD_EINSUM)
        if return_logits:
            raise ValueError("return_logits=True is not built for GraphIsoConvTD (no branch sum without the ReLU)")
        if not isinstance(kernel_size, int) or not 1 <= kernel_size <= 8:
            raise ValueError("kernel_size must be an int in 1..8, got %r" % (kernel_size,))
        self.filters, self.kernel_size, self.return_logits, self.einsum = list(filters), kernel_size, False, einsum
        self.mlps = torch.nn.ModuleList(_mlp(self.filters, 4, False) for _ in range(kernel_size))
        self.register_parameter("epsilon", None)

    _first_kernel = "mlps.0.0.kernel"

    def _all_layers(self):
        return [list(m) for m in self.mlps]

    def forward(self, x, A, training=None):
        _require(x, 4, "x (B, C, T, V)")
        _require(A, 3, "A (kernel_size - 1, V, V)")
        B, C, T, V = x.shape
        K = self.kernel_size
        if tuple(A.shape) != (K - 1, V, V):
            raise ValueError("A must be (kernel_size - 1, V, V) = (%d, %d, %d), got %s" % (K - 1, V, V, tuple(A.shape)))
        _dense_limits(K, V)
        if B * T * V >= 1 << 22:
            raise ValueError("B * T * V = %d columns: the convolutions are built for fewer than 2^22" % (B * T * V))
        return self._call(_GraphIsoConvTDFn, x, A, training)
