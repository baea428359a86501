"""Drop-in for the reference's models/stgcn_debug.py: `Model(num_classes=60)` called as `model(x, training)` -- ST-GCN whose blocks
contract with a trainable adjacency PER FRAME (SGTACN, models/stgcn_debug.py:118-145: einsum 'nkctv,ktvw->nctw'), one table
`l{i}.adjacency_matrix` of shape (3, T_i, 25, 25) per block, initialised to Graph().A repeated over the block's input frames
(`main_gnn.py --model stgcn_debug --freeze-graph-until E`: the tables are trained only while epoch > E).

x: (N, in_channels=3, T=frames, V=25, M) float32 on the GPU -> logits (N, num_classes).
The arithmetic runs in libsar_hip.so through sar_amd.stgcn_ta.STGCNTA; this module adapts it to torch.nn.Module / autograd exactly
like models/stpgcn.py does.  `trainable_adjacency` is accepted for main_gnn.py's sake: this model always owns its tables.

The reference file's two pooling-side layers are here too (fp32, contiguous float32 CUDA tensors; anything else is a ValueError):

  GPool(keeprate)               forward(x (N,C,T,V), A (N,K,V,V), training) -> (x (N,C,T,keep), A (N,K,keep,keep))   :29-72
  SGCN(filters, kernel_size=3)  forward(x (N,C,T,V), A (N,K,V,V), training) -> (x (N,filters,T,V), A)                :93-115

GPool is the top-k pooling of Graph U-Nets on csrc/gpool.hip (sar_amd.ops.gpool_forward / gpool_backward; V <= 64, K <= 8, N <= 65535):
keep = int(float32(keeprate) * float32(V)) vertices of largest projection onto the trainable `projection_vector` (C T, 1), created on
the first call (glorot uniform) or by load_state_dict, scaled by the sigmoid of their score; A becomes the gathered second power.
SGCN is Conv2D(K filters, 1x1) then einsum 'nkctv,nkvw->nctw' with the per-sample adjacency GPool emits, Keras parameters `kernel`
(1, 1, C, K filters) / `bias` as GraphConvTD.  It runs the per-frame kernels of csrc/graph_dense_t.hip with the roles of frame and
sample exchanged (columns ordered (t, n, v), table At[k, n] = A[n, k]): K <= 4, V <= 32, K V <= 76, T <= 65535 (the kernels'
sample axis is a 16-bit grid axis), N T V < 2^22 (the 1x1 product).
"""
import math

import torch

from sar_amd import ops
from sar_amd.stgcn_ta import STGCNTA  # noqa: F401
from models.gcn import _Conv1x1Layer, _ConvContractFn, _require
from models.stgcn import _STGCNFunction, _Variable


class Model(torch.nn.Module):
    def __init__(self, num_classes=60, in_channels=3, device="cuda", seed=0, stream="joint", mfma="fp32",
                 trainable_adjacency=True, frames=300):
        super().__init__()
        assert stream in ("joint", "bone", "joint_motion", "bone_motion"), stream
        assert mfma == "fp32", "models.stgcn_debug runs in fp32"
        from sar_amd.bone import NTU_BONE_PAIRS
        self.engine = STGCNTA(num_classes=num_classes, in_channels=in_channels, device=device, seed=seed, frames=frames,
                              bone_pairs=NTU_BONE_PAIRS if stream.startswith("bone") else None, motion=stream.endswith("motion"))
        self._names = list(self.engine.shapes)
        for k in self._names:
            self.register_parameter(k.replace(".", "_"), torch.nn.Parameter(self.engine.p[k]))

    @property
    def trainable_variables(self):
        return [_Variable(k, getattr(self, k.replace(".", "_"))) for k in self._names]

    @property
    def variables(self):
        return self.trainable_variables

    @property
    def adjacency_matrices(self):
        """the per-block tables, (3, T_i, 25, 25) each"""
        return [getattr(self, self.engine.table_name(i).replace(".", "_")) for i in range(len(self.engine.blocks))]

    def forward(self, x, training=None):
        if training is None:
            training = self.training
        params = [getattr(self, k.replace(".", "_")) for k in self._names]
        if training and torch.is_grad_enabled():
            return _STGCNFunction.apply(x, self.engine, True, *params)
        return self.engine.forward(x, training=training)

    def train_step(self, x, labels, lr, global_batch_size=None, momentum=0.9):
        logits, loss = self.engine.loss_and_grad(x, labels, global_batch_size)
        self.engine.sgd_step(lr, momentum)
        return logits, loss


class _GPoolFn(torch.autograd.Function):
    """the whole layer: gradients for x, A and projection_vector; none through the selection"""

    @staticmethod
    def forward(ctx, x, A, p, keeprate):
        out, A_out, saved = ops.gpool_forward(x, A, p, keeprate)
        ctx.set_materialize_grads(False)              # an output nobody differentiates arrives as None, not as zeros
        ctx.save_for_backward(x, A, *saved)
        ctx.p_shape = tuple(p.shape)
        return out, A_out

    @staticmethod
    def backward(ctx, dout, dA_out):
        x, A = ctx.saved_tensors[:2]
        need_x, need_A, need_p = ctx.needs_input_grad[:3]
        dx, dp, dA = ops.gpool_backward(x, A, tuple(ctx.saved_tensors[2:]),
                                        dout.contiguous() if (dout is not None and (need_x or need_p)) else None,
                                        dA_out.contiguous() if (dA_out is not None and need_A) else None)
        return dx if need_x else None, dA, dp.view(ctx.p_shape) if (dp is not None and need_p) else None, None


class GPool(torch.nn.Module):
    """models/stgcn_debug.py:29-72: top-k graph pooling with the trainable `projection_vector` (C T, 1)"""

    def __init__(self, keeprate):
        super().__init__()
        if not (isinstance(keeprate, (int, float)) and 0.0 < float(keeprate) <= 1.0):
            raise ValueError("keeprate must be in (0, 1], got %r" % (keeprate,))
        self.keeprate = float(keeprate)
        self.register_parameter("projection_vector", None)

    def build(self, C, T, device):
        if self.projection_vector is None:
            lim = math.sqrt(6.0 / (C * T + 1))                       # glorot uniform of a (C T, 1) kernel
            self.projection_vector = torch.nn.Parameter(((torch.rand(C * T, 1, dtype=torch.float64) * 2 - 1) * lim).to(torch.float32).to(device))
        elif self.projection_vector.shape[0] != C * T:
            raise ValueError("the layer was built for C * T = %d, got C = %d, T = %d" % (self.projection_vector.shape[0], C, T))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        p = state_dict.get(prefix + "projection_vector")
        if self.projection_vector is None and p is not None:
            self.projection_vector = torch.nn.Parameter(torch.empty(tuple(p.shape), dtype=torch.float32, device=p.device if p.is_cuda else "cuda"))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x, A, training=False):
        _require(x, 4, "x (N, C, T, V)")
        if not (isinstance(A, torch.Tensor) and A.dim() == 4):
            raise ValueError("A must be 4-D: expand a (K, V, V) or (N, V, V) adjacency to (N, K, V, V)")
        _require(A, 4, "A (N, K, V, V)")
        N, C, T, V = x.shape
        if tuple(A.shape) != (N, A.shape[1], V, V):
            raise ValueError("A must be (N, K, V, V) = (%d, K, %d, %d), got %s" % (N, V, V, tuple(A.shape)))
        if V > ops.GPOOL_VMAX or A.shape[1] > ops.GPOOL_KMAX:
            raise ValueError("GPool is built for V <= %d and K <= %d (got V = %d, K = %d)" % (ops.GPOOL_VMAX, ops.GPOOL_KMAX, V, A.shape[1]))
        ops.gpool_keep(self.keeprate, V)
        self.build(C, T, x.device)
        return _GPoolFn.apply(x, A, self.projection_vector, self.keeprate)


def _to_cn_tnv(x):
    """(N, C, T, V) -> CN matrix [C][(t, n, v)]: in NCHW the pair (c, t) is one index of stride V"""
    N, C, T, V = x.shape
    out = torch.empty((C, T * N * V), dtype=torch.float32, device=x.device)
    ops.permute3(x, out, C * T, N, V, V, C * T * V, 1)
    return out


def _from_cn_tnv(m, shape):
    """CN matrix [F][(t, n, v)] -> contiguous (N, F, T, V) = shape"""
    N, F, T, V = shape
    out = torch.empty(shape, dtype=torch.float32, device=m.device)
    ops.permute3(m, out, N, F * T, V, V, N * V, 1)
    return out


class _Swap01Fn(torch.autograd.Function):
    """(a, b, ...) -> contiguous (b, a, ...) with sar_permute3_f32; its own inverse, so also its gradient"""

    @staticmethod
    def forward(ctx, t):
        a, b = t.shape[:2]
        inner = t.numel() // (a * b)
        out = torch.empty((b, a) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
        ops.permute3(t, out, b, a, inner, inner, b * inner, 1)
        return out

    @staticmethod
    def backward(ctx, d):
        return _Swap01Fn.apply(d.contiguous())


# the per-frame contraction of csrc/graph_dense_t.hip, dims (K, F, V, B, T), on columns (t, n, v) with B := T, T := N and the table
# At (K, N, V, V): the "frame" is the sample, and its dadj -- summed over channels and over what it calls samples -- the per-sample dA
DENSE_T_CONTRACTION = (ops.graph_dense_t_fwd, ops.graph_dense_t_bwd_data, ops.graph_dense_t_dA)


class SGCN(_Conv1x1Layer):
    """models/stgcn_debug.py:93-115: Conv2D(kernel_size * filters, 1x1), then einsum 'nkctv,nkvw->nctw' with a per-sample adjacency"""

    def __init__(self, filters, kernel_size=3):
        super().__init__(filters * kernel_size, 4)
        self.filters, self.kernel_size = int(filters), int(kernel_size)

    def forward(self, x, A, training=None):
        _require(x, 4, "x (N, C, T, V)")
        _require(A, 4, "A (N, K, V, V)")
        N, C, T, V = x.shape
        K = self.kernel_size
        if tuple(A.shape) != (N, K, V, V):
            raise ValueError("A must be (N, K, V, V) = (%d, %d, %d, %d), got %s" % (N, K, V, V, tuple(A.shape)))
        if K > 4 or V > 32 or K * V > 76:
            raise ValueError("SGCN is built for K <= 4, V <= 32 and K * V <= 76 (got K = %d, V = %d)" % (K, V))
        if T > 65535 or N * T * V >= 1 << 22:
            raise ValueError("SGCN is built for T <= 65535 frames (a 16-bit grid axis of the contraction) and N * T * V < 2^22 columns "
                             "(the 1x1 product); got N = %d, T = %d, V = %d" % (N, T, V))
        self.build(C, x.device)
        return _ConvContractFn.apply(x, _Swap01Fn.apply(A), self.kernel, self.bias, DENSE_T_CONTRACTION, (K, self.filters, V, T, N),
                                     self.filters, dict(B=T, V=V, T_src=N, T_out=N), (_to_cn_tnv, _from_cn_tnv)), A
