"""Layer-level drop-in for the reference's models/stpgcnp.py:11-38: `ProjectionGraphPool` as a torch module whose arithmetic runs in
libsar_hip.so (csrc/pgpool.hip, fp32).

  ProjectionGraphPool(vertices)     forward(x (N, C, ...), A, training=None) -> (z (N, C, J), A_out (N, J, J))

x may have any trailing dimensions: they are flattened to P columns per sample (the reference's reshape to (N, C, -1, 1)).  The
incoming A is ignored, as in the reference.  With s = sigmoid(variance):

    d   = sum_c ((x[c,p] - centers[c,j]) / s[c,j])^2                  (P, J) per sample
    q   = softmax_j(-0.5 max(d, 1e-12));  qs = sum_p q
    zp  = (x q^T - centers qs) / (s qs)                               (C, J)
    z   = zp * rsqrt(max(sum_j zp^2, 1e-12))                          l2_normalize over the LAST axis (J)
    A_out = z^T z

The literal formulation holds (x - centers) / s for all vertices at once -- (N, C, P, J), 64 GB at N = 128, C = 256, P = 950,
J = 512; the kernels never form it (nothing with both a P and a C x J extent is written).  A vertex no column is assigned to
(qs == 0) gives 0 / 0 = NaN, as in the reference: there is no guard.

Parameters `centers` and `variance`, each (1, C, 1, J), are created on the first call as Keras' `build` does (or by
load_state_dict) with Keras' default glorot_uniform.  Inputs are contiguous float32 CUDA tensors; anything else -- and C or
vertices above 512 -- raises ValueError before a launch.  Each call is ONE torch.autograd.Function; its backward takes the
gradients of both outputs and yields dx, dcenters and dvariance.  The layer converts (N, C, P) <-> the kernels' CN layout
([C][N * P]) at its boundary with the permute kernel (models/gcn.py: to_cn / from_cn).
"""
import torch

from sar_amd import ops
from sar_amd.stpgcn import glorot_uniform

from .gcn import from_cn, to_cn


class _ProjectionGraphPoolFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, centers, variance):
        B, C = x.shape[:2]
        P = x.numel() // (B * C)
        X = to_cn(x)
        zn, A, saved = ops.pgpool_forward(X, B, P, centers, variance)
        ctx.save_for_backward(X, centers, zn, *saved)
        ctx.shape = tuple(x.shape)
        return zn, A

    @staticmethod
    def backward(ctx, dz, dA):
        X, centers, zn = ctx.saved_tensors[:3]
        saved = ctx.saved_tensors[3:]
        B, C = ctx.shape[:2]
        P = X.shape[1] // B
        dX = torch.empty_like(X)
        dcen, dvar = torch.empty_like(centers), torch.empty_like(centers)
        ops.pgpool_backward(X, B, P, centers, zn, saved, None if dz is None else dz.contiguous(), None if dA is None else dA.contiguous(),
                            dX, dcen, dvar)
        return from_cn(dX, ctx.shape), dcen, dvar


class ProjectionGraphPool(torch.nn.Module):
    """models/stpgcnp.py:11-38; `centers`, `variance` (1, C, 1, vertices)"""

    def __init__(self, vertices):
        super().__init__()
        if not isinstance(vertices, int) or not 1 <= vertices <= ops.PGPOOL_MAX:
            raise ValueError("vertices must be an int in 1..%d, got %r" % (ops.PGPOOL_MAX, vertices))
        self.vertices = vertices
        self.register_parameter("centers", None)
        self.register_parameter("variance", None)

    def build(self, in_channels, device):
        if self.centers is None:
            shape = (1, int(in_channels), 1, self.vertices)
            for name in ("centers", "variance"):      # (generator None: torch's global one, as models/gcn.py draws its kernels)
                setattr(self, name, torch.nn.Parameter(glorot_uniform(shape, None).to(torch.float32).to(device)))
        elif self.centers.shape[1] != in_channels:
            raise ValueError("the layer was built for %d input channels, got %d" % (self.centers.shape[1], in_channels))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        c = state_dict.get(prefix + "centers")
        if self.centers is None and c is not None:
            self.build(c.shape[1], c.device if c.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x, A=None, training=None):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous()):
            raise ValueError("x (N, C, ...) must be a contiguous float32 CUDA tensor with at least 2 dimensions")
        N, C = x.shape[:2]
        if not 1 <= C <= ops.PGPOOL_MAX or x.numel() == 0:
            raise ValueError("ProjectionGraphPool is built for 1 <= C <= %d and a non-empty x (got shape %s)" % (ops.PGPOOL_MAX, tuple(x.shape)))
        if x.numel() // C >= 1 << 31 or N > 65535:
            raise ValueError("N = %d samples of %d columns: built for N <= 65535 and fewer than 2^31 columns" % (N, x.numel() // (N * C)))
        self.build(C, x.device)
        return _ProjectionGraphPoolFn.apply(x, self.centers, self.variance)
