"""The adaptive adjacency of 2s-AGCN as torch modules on the HIP kernels (fp32): the producer of the per-sample adjacency at full joint
resolution that `models.stgcn_debug.SGCN` consumes.  The reference has no counterpart; it takes its graph construction, its data
pipeline and its bone and motion streams from that code base, where each subset's adjacency is A_k + B_k + C_k.  A_k is the fixed
table, B_k is `AdjGraphConv` / --trainable-adjacency, and C_k is this module:

  AdaptiveAdjacency(embed_channels, kernel_size=3)               forward(x (N,C,T,V), A (K,V,V), training) -> A_eff (N,K,V,V)
  AdaptiveGraphConv(filters, kernel_size=3, embed_channels=None) forward(x (N,C,T,V), A (K,V,V), training) -> (y (N,filters,T,V), A)

  theta = Conv1x1(K Ce, no bias)(x)     phi = Conv1x1(K Ce, bias)(x)            Ce = embed_channels, channel k Ce + e belongs to subset k
  A_eff[n,k] = A[k] + softmax over v of (1 / (Ce T)) sum_{e,t} theta[n, k Ce + e, t, v] phi[n, k Ce + e, t, w]      (every column sums to 1)

theta has no bias: a bias b_e adds b_e sum_t phi[e, t, w] to every v of a column, which the softmax over v removes, so its gradient is
identically zero.  AdaptiveAdjacency is ONE autograd node over sar_amd.ops.adjattn_forward / adjattn_backward (csrc/adjattn.hip: the
similarity and the embeddings' gradients on the fp32 MFMA pipe, reading theta and phi where they lie; theta and phi one 1x1 product on
the stacked kernel), with gradients for x, the three parameters and A -- so A may be a trainable A + B.  Parameters `theta.kernel`,
`phi.kernel` (1, 1, C, K Ce) and `phi.bias` (K Ce) in the Keras layouts, created on the first call (or by load_state_dict) with
VarianceScaling(2, fan_out, truncated_normal) and a zero bias, as every 1x1 layer of models/gcn.py.  Under no_grad, or when nothing
requires a gradient, nothing is saved.  AdaptiveGraphConv is AdaptiveAdjacency followed by SGCN(filters, kernel_size) on A_eff, two
autograd nodes; it takes GraphConvTD's place in a body and hands the A it was given on.

Limits (ValueError before anything is built or launched): contiguous float32 CUDA tensors, 1 <= V <= 32, 1 <= K <= 4, 1 <= K Ce <= 512,
N T V < 2^22 (the 1x1 product), N K <= 65535, A of shape (kernel_size, V, V); AdaptiveGraphConv also SGCN's K V <= 76 and T <= 65535.
`training` changes nothing (no dropout, no BatchNorm) and is kept for the signature."""
import torch

from models.gcn import _require, from_cn, to_cn, variance_scaling_
from models.stgcn_debug import SGCN
from sar_amd import ops


class _AdaptiveAdjacencyFn(torch.autograd.Function):
    """the whole layer as one node: gradients for x, A, theta.kernel, phi.kernel, phi.bias"""

    @staticmethod
    def forward(ctx, x, A, theta_kernel, phi_kernel, phi_bias, save):
        N, _, T, V = x.shape
        X = to_cn(x)
        A_eff, saved = ops.adjattn_forward(X, N, T, V, A, theta_kernel, phi_kernel, phi_bias)
        if save:
            ctx.save_for_backward(X, *saved, theta_kernel, phi_kernel)
            ctx.shape = tuple(x.shape)
        return A_eff

    @staticmethod
    def backward(ctx, dA_eff):
        X, E, P, theta_kernel, phi_kernel = ctx.saved_tensors
        N, _, T, V = ctx.shape
        need_x, need_A = ctx.needs_input_grad[:2]
        dX, dtk, dpk, dpb, dA = ops.adjattn_backward(X, N, T, V, (E, P), theta_kernel, phi_kernel, dA_eff.contiguous(), need_dx=need_x,
                                                     need_dA=need_A)
        return (from_cn(dX, ctx.shape) if need_x else None), dA, dtk, dpk, dpb, None


class _Embedding(torch.nn.Module):
    """Conv2D(out_channels, 1x1, use_bias)'s variables in the Keras layouts -- kernel (1, 1, C, out_channels), bias (out_channels) --,
    created on the first call (or by load_state_dict) as models.gcn._Conv1x1Layer creates them"""

    def __init__(self, out_channels, use_bias):
        super().__init__()
        self.out_channels, self.use_bias = int(out_channels), bool(use_bias)
        self.register_parameter("kernel", None)
        if self.use_bias:
            self.register_parameter("bias", None)

    def build(self, in_channels, device):
        if self.kernel is None:
            self.kernel = torch.nn.Parameter(torch.empty((1, 1, int(in_channels), self.out_channels), dtype=torch.float32, device=device))
            variance_scaling_(self.kernel)
            if self.use_bias:
                self.bias = torch.nn.Parameter(torch.zeros(self.out_channels, dtype=torch.float32, device=device))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if self.kernel is None and k is not None:
            self.build(k.shape[-2], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class AdaptiveAdjacency(torch.nn.Module):
    """see the module docstring.  forward(x (N, C, T, V), A (K, V, V), training=None) -> A_eff (N, K, V, V)"""

    def __init__(self, embed_channels, kernel_size=3):
        super().__init__()
        Ce, K = int(embed_channels), int(kernel_size)
        if not (1 <= K <= ops.ADJATTN_KMAX and 1 <= Ce and K * Ce <= ops.ADJATTN_EMAX):
            raise ValueError("the kernels are built for 1 <= K <= %d and 1 <= K Ce <= %d (got kernel_size = %d, embed_channels = %d)"
                             % (ops.ADJATTN_KMAX, ops.ADJATTN_EMAX, K, Ce))
        self.embed_channels, self.kernel_size = Ce, K
        self.theta, self.phi = _Embedding(K * Ce, False), _Embedding(K * Ce, True)

    def check(self, x, A):
        """every limit of the layer: ValueError before a parameter is built or a kernel launched"""
        _require(x, 4, "x (N, C, T, V)")
        _require(A, 3, "A (K, V, V)")
        N, C, T, V = x.shape
        K = self.kernel_size
        if tuple(A.shape) != (K, V, V):
            raise ValueError("A must be (K, V, V) = (%d, %d, %d), got %s" % (K, V, V, tuple(A.shape)))
        if min(N, C, T, V) < 1 or V > ops.ADJATTN_VMAX:
            raise ValueError("need a non-empty x with V <= %d, got %s" % (ops.ADJATTN_VMAX, tuple(x.shape)))
        if N * T * V >= 1 << 22 or N * K > 65535:
            raise ValueError("AdaptiveAdjacency is built for N T V < 2^22 columns (the 1x1 product) and N K <= 65535 (got N = %d, T = %d, "
                             "V = %d, K = %d)" % (N, T, V, K))
        for layer in (self.theta, self.phi):
            if layer.kernel is not None and layer.kernel.shape[-2] != C:
                raise ValueError("the layer was built for %d input channels, got %d" % (layer.kernel.shape[-2], C))

    def forward(self, x, A, training=None):
        self.check(x, A)
        self.theta.build(x.shape[1], x.device)
        self.phi.build(x.shape[1], x.device)
        ts = (x, A, self.theta.kernel, self.phi.kernel, self.phi.bias)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in ts)
        return _AdaptiveAdjacencyFn.apply(*ts, save)


class AdaptiveGraphConv(torch.nn.Module):
    """AdaptiveAdjacency, then SGCN(filters, kernel_size) on A_eff; embed_channels=None means max(filters // 4, 1).  Parameters
    `adjacency.theta.kernel`, `adjacency.phi.kernel`, `adjacency.phi.bias`, `gcn.kernel` (1, 1, C, K filters), `gcn.bias`"""

    def __init__(self, filters, kernel_size=3, embed_channels=None):
        super().__init__()
        self.filters, self.kernel_size = int(filters), int(kernel_size)
        self.adjacency = AdaptiveAdjacency(max(self.filters // 4, 1) if embed_channels is None else embed_channels, kernel_size)
        self.gcn = SGCN(filters, kernel_size)

    def forward(self, x, A, training=None):
        self.adjacency.check(x, A)
        N, C, T, V = x.shape
        if self.kernel_size * V > 76 or T > 65535:
            raise ValueError("SGCN is built for K * V <= 76 and T <= 65535 (got K = %d, V = %d, T = %d)" % (self.kernel_size, V, T))
        if self.gcn.kernel is not None and self.gcn.kernel.shape[-2] != C:
            raise ValueError("the layer was built for %d input channels, got %d" % (self.gcn.kernel.shape[-2], C))
        y, _ = self.gcn(x, self.adjacency(x, A, training), training)
        return y, A
