"""Drop-in for the reference's models/stgcn.py: `Model(num_classes=60)` called as `model(x, training)`.

x: (N, in_channels=3, T, V=25, M) float32 on the GPU -> logits (N, num_classes)   (models/stgcn.py:135-160).
The arithmetic runs in libsar_hip.so through sar_amd.stgcn.STGCN; this module only adapts it to the
torch.nn.Module / autograd interfaces so that `loss.backward()` and any torch optimizer work, and keeps the
reference's attribute names used by its training script (main_gnn.py:228-232,311,315):
  * `trainable_variables` -- objects with a `.name`; the adjacency is exposed as the NON-trainable
    variable `adjacency_matrix` (models/stgcn.py:105-109),
  * block hyper-parameters (models/stgcn.py:113-123) are fixed as in the reference.

`SpatioTemporalGraphConv` (models/stgcn.py:11-64) is the block as a layer of its own, for bodies that are not pre-built: one
autograd node whose forward and backward are the ENGINE's block code (STGCN.block_forward / block_backward on a one-block engine:
the folded BN + ReLU prologue of the temporal convolution, the statistics epilogues, bn_add_relu with the 1-bit mask and the matching
backward passes).  It converts NCHW <-> CN at its boundary and copies its parameters into the engine per call, so a network composed
of these layers pays that per layer where `Model` does not: an interface, not the fast path.

`TemporalAttention(num_hidden)` (models/stgcn.py:67-85) is the per-frame gate: an MLP over the V C features of a frame ends in
Dense(1, sigmoid), and every joint and channel of the frame is multiplied by the result.  One autograd node over
sar_amd.ops.tattn_forward / tattn_backward (csrc/tattn.hip): the first Dense, its weight gradient and the input gradient are fp32 MFMA
kernels that read x where it lies (no transposed copy), the later layers are the library's 1x1 products.  Not wired into main_gnn.py
(the reference wires it into no model); in front of `Model` it trains under one optimizer, the engines return d loss / d clip.
"""
import math

import numpy as np
import torch

from models.gcn import GraphConvTD, _require, from_cn, to_cn, variance_scaling_
from sar_amd import ops
from sar_amd.graph_tables import gather_lists
from sar_amd.stgcn import STGCN, BLOCKS, KS, KT  # noqa: F401


class _STGCNFunction(torch.autograd.Function):
    """Whole-network forward/backward on the HIP engine (one autograd node)."""

    @staticmethod
    def forward(ctx, x, engine, training, *params):
        ctx.engine = engine
        ctx.training = training
        return engine.forward(x, training=training)

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.engine
        if not ctx.training:
            raise RuntimeError("backward through model(x, training=False) is not supported (inference path)")
        # d loss / d x only when x asks for it (a leaf with requires_grad, or a learned front end such as TemporalSampler)
        dx = eng.backward(dlogits.contiguous(), need_dx=ctx.needs_input_grad[0])
        grads = tuple(eng.g[k].clone() for k in eng.shapes)
        return (dx, None, None) + grads


class _Variable:
    """Keras-like view of a parameter: `.name`, `.numpy()`; `.tensor` is the torch parameter."""

    def __init__(self, name, tensor, trainable=True):
        self.name, self.tensor, self.trainable = name, tensor, trainable

    def numpy(self):
        return self.tensor.detach().cpu().numpy()


class Model(torch.nn.Module):
    def __init__(self, num_classes=60, in_channels=3, device="cuda", seed=0, stream="joint", mfma="fp32",
                 trainable_adjacency=False, blocks=None):
        """stream (not in the reference's constructor, which reads pre-computed files): 'joint', 'bone', 'joint_motion'
        or 'bone_motion' -- the bone (data_gen/gen_bone_data.py) and motion (data_gen/gen_motion_data.py) transforms are
        applied on the fly to JOINT input inside the data_bn prologue, bit-exactly.
        blocks (not in the reference's constructor either): another stack of (filters, stride, residual) than the reference's ten.
        mfma: 'fp32' (the reference's arithmetic on the fp32 MFMA), 'f32_split' (fp32 storage and results, the contractions as three
        products of fp16 terms on the fp16 matrix pipe: same parity tolerances, 1.6x the training rate; 'f32_split_bf16x6': six
        products of bf16 terms) or 'bf16' (bf16 activations and MFMA operands, fp32 everything else: sar_amd/stgcn.py)."""
        super().__init__()
        assert stream in ("joint", "bone", "joint_motion", "bone_motion"), stream
        from sar_amd.bone import NTU_BONE_PAIRS
        self.engine = STGCN(num_classes=num_classes, in_channels=in_channels, device=device, seed=seed,
                            bone_pairs=NTU_BONE_PAIRS if stream.startswith("bone") else None,
                            motion=stream.endswith("motion"), mfma=mfma, trainable_adjacency=trainable_adjacency, blocks=blocks)
        # parameters are views into the engine's flat fp32 buffer (one all-reduce bucket, fused optimizer)
        self._names = list(self.engine.shapes)
        for k in self._names:
            self.register_parameter(k.replace(".", "_"), torch.nn.Parameter(self.engine.p[k]))
        if not trainable_adjacency:
            self.register_buffer("adjacency_matrix", self.engine.A)      # non-trainable, models/stgcn.py:105-109
        # trainable_adjacency=True (models/gcn.py:212-238 AdjGraphConv's variable, shared by the blocks): `adjacency_matrix`
        # is one of the parameters registered above and main_gnn.py's --freeze-graph-until gates its gradient
        self.A = self.adjacency_matrix

    @property
    def trainable_variables(self):
        return [_Variable(k, getattr(self, k.replace(".", "_"))) for k in self._names]

    @property
    def variables(self):
        return self.trainable_variables + [_Variable("adjacency_matrix", self.adjacency_matrix, False)]

    def forward(self, x, training=None):
        if training is None:
            training = self.training
        params = [getattr(self, k.replace(".", "_")) for k in self._names]
        if training and torch.is_grad_enabled():
            return _STGCNFunction.apply(x, self.engine, True, *params)
        return self.engine.forward(x, training=training)

    # the engine's fused paths, for scripts that want the reference's exact train step without autograd
    def train_step(self, x, labels, lr, global_batch_size=None, momentum=0.9):
        logits, loss = self.engine.loss_and_grad(x, labels, global_batch_size)
        self.engine.sgd_step(lr, momentum)
        return logits, loss


class _BlockFunction(torch.autograd.Function):
    """one ST-GCN block on the engine's block forward / backward (one autograd node)"""

    @staticmethod
    def forward(ctx, x, A, layer, eng, *params):
        B, C, T, V = x.shape
        y, To, sb = eng.block_forward(0, to_cn(x), B, T, True)
        ctx.layer, ctx.eng, ctx.sb, ctx.call, ctx.shape = layer, eng, sb, layer._calls, (B, C, T, V)
        return from_cn(y, (B, y.shape[0], To, V))

    @staticmethod
    def backward(ctx, dout):
        layer, eng = ctx.layer, ctx.eng
        if ctx.call != layer._calls:
            raise RuntimeError("SpatioTemporalGraphConv was called again (training or inference: either overwrites the block's "
                               "BatchNorm state) before this call's backward; use one layer instance per position and run "
                               "evaluation calls after backward")
        dX = eng.block_backward(0, ctx.sb, to_cn(dout.contiguous()), ctx.shape[0])
        dA = eng.g["adjacency_matrix"].clone() if (eng.dense_A and ctx.needs_input_grad[1]) else None
        grads = tuple(eng.g[k].clone() for k in layer._engine_names())
        return ((from_cn(dX, ctx.shape) if ctx.needs_input_grad[0] else None), dA, None, None) + grads


class SpatioTemporalGraphConv(torch.nn.Module):
    """models/stgcn.py:11-64: GraphConvTD -> BN -> ReLU -> Conv2D([9, 1], stride) -> BN, plus the residual (none / identity / strided
    1x1 convolution + BN, decided on the first call), add, ReLU.  forward(x (B,C,T,V), A (3,V,V), training) -> (x (B,filters,T/s,V), A).
    Parameters in the Keras layouts: sgcn.kernel / sgcn.bias (the GraphConvTD it owns), bn1_*, tcn_kernel (9, 1, f, f) / tcn_bias, bn2_*,
    res_kernel (1, 1, C, f) / res_bias / res_bn_*; moving statistics are buffers with the engine's eps, momentum and unbiased moving
    variance.  training=False uses the moving statistics and updates nothing.  A that requires a gradient (or is denser than 4
    non-zeros per column / row) takes the engine's dense path, which yields dA (V <= 32).
    The engine behind the layer keeps ONE set of BatchNorm scales, shifts and batch statistics, which backward reads: any later call
    of the same instance -- a training=False call included, since inference overwrites the folded scale and shift -- before a
    training call's backward makes that backward raise RuntimeError."""

    def __init__(self, filters, kernel_size=(3, 9), stride=1, activation="relu", residual=True):
        super().__init__()
        if activation != "relu":
            raise ValueError("activation %r is not implemented (only 'relu' is)" % (activation,))
        if tuple(kernel_size) != (KS, KT):
            raise ValueError("kernel_size %r is not built (only [%d, %d] is)" % (kernel_size, KS, KT))
        self.filters, self.stride, self.residual = int(filters), int(stride), bool(residual)
        self.sgcn = GraphConvTD(filters, kernel_size=KS)
        self.kind = None
        self._engines, self._tables_of, self._calls = {}, None, 0

    # ---- parameters (created on the first call, or by load_state_dict)
    def _bn(self, name, C, device):
        self.register_parameter(name + "_gamma", torch.nn.Parameter(torch.ones(C, dtype=torch.float32, device=device)))
        self.register_parameter(name + "_beta", torch.nn.Parameter(torch.zeros(C, dtype=torch.float32, device=device)))
        self.register_buffer(name + "_moving_mean", torch.zeros(C, dtype=torch.float32, device=device))
        self.register_buffer(name + "_moving_var", torch.ones(C, dtype=torch.float32, device=device))

    def _conv(self, name, shape, device):
        k = torch.nn.Parameter(torch.empty(shape, dtype=torch.float32, device=device))
        variance_scaling_(k)
        self.register_parameter(name + "_kernel", k)
        self.register_parameter(name + "_bias", torch.nn.Parameter(torch.zeros(shape[-1], dtype=torch.float32, device=device)))

    def build(self, in_channels, device, kind=None):
        if self.kind is not None:
            if self.sgcn.kernel.shape[-2] != in_channels:
                raise ValueError("the block was built for %d input channels, got %d" % (self.sgcn.kernel.shape[-2], in_channels))
            return
        f = self.filters
        self.cin = int(in_channels)
        # models/stgcn.py:41-56
        self.kind = kind or ("none" if not self.residual else ("identity" if (in_channels == f and self.stride == 1) else "conv"))
        self.sgcn.build(in_channels, device)
        self._bn("bn1", f, device)
        self._conv("tcn", (KT, 1, f, f), device)
        self._bn("bn2", f, device)
        if self.kind == "conv":
            self._conv("res", (1, 1, in_channels, f), device)
            self._bn("res_bn", f, device)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "sgcn.kernel")
        if self.kind is None and k is not None:
            kind = "conv" if prefix + "res_kernel" in state_dict else ("none" if not self.residual else "identity")
            self.build(k.shape[-2], k.device if k.is_cuda else "cuda", kind)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _names(self):
        """(engine name, this module's tensor) of every trainable parameter, in the engine's order"""
        out = [("l0.gcn.kernel", self.sgcn.kernel), ("l0.gcn.bias", self.sgcn.bias)]
        for e, m in (("bn1.gamma", "bn1_gamma"), ("bn1.beta", "bn1_beta"), ("tcn.kernel", "tcn_kernel"), ("tcn.bias", "tcn_bias"),
                     ("bn2.gamma", "bn2_gamma"), ("bn2.beta", "bn2_beta")):
            out.append(("l0." + e, getattr(self, m)))
        if self.kind == "conv":
            for e, m in (("res.kernel", "res_kernel"), ("res.bias", "res_bias"), ("res_bn.gamma", "res_bn_gamma"),
                         ("res_bn.beta", "res_bn_beta")):
                out.append(("l0." + e, getattr(self, m)))
        return out

    def _engine_names(self):
        return [k for k, _ in self._names()]

    # ---- the one-block engine behind the layer
    def _engine(self, A, V, device):
        """the engine for this A: gather tables for a fixed sparse A (rebuilt when A is another tensor or was edited in place; the
        tensor is kept, so its address cannot be reused by another), the dense path otherwise"""
        dense = A.requires_grad
        if not dense:
            key = (A.data_ptr(), A._version)
            if self._tables_of is None or self._tables_of[0] is not A or self._tables_of[1] != key:
                host = A.detach().cpu().numpy().astype(np.float64)
                try:                     # checked on the host first: a dense A must not leave the engine's tables half replaced
                    gather_lists(host.astype(np.float32), False), gather_lists(host.astype(np.float32), True)
                    tables = True
                except ValueError:       # denser than the gather lists hold
                    tables = False
                if tables and False in self._engines:
                    self._engines[False]._init_adjacency(host)
                elif tables:
                    self._engines[False] = self._make_engine(host, V, device, False)
                self._tables_of = (A, key, tables)
            dense = not self._tables_of[2]
        if dense:
            if V > 32:
                raise ValueError("the dense adjacency path is built for V <= 32 (got %d)" % V)
            if True not in self._engines:
                self._engines[True] = self._make_engine(np.zeros((KS, V, V)), V, device, True)
            eng = self._engines[True]
            eng.train_adjacency = bool(A.requires_grad)
            eng.p["adjacency_matrix"].copy_(A.detach())
        else:
            eng = self._engines[False]
        with torch.no_grad():
            for k, t in self._names():
                eng.p[k].copy_(t)
        for name in ("bn1", "bn2") + (("res_bn",) if self.kind == "conv" else ()):     # the statistics ARE this module's buffers
            eng.bn["l0." + name].moving_mean = getattr(self, name + "_moving_mean")
            eng.bn["l0." + name].moving_var = getattr(self, name + "_moving_var")
        return eng

    def _make_engine(self, A_host, V, device, dense):
        eng = STGCN(num_classes=4, in_channels=self.cin, num_node=V, A=A_host, device=device,
                    blocks=[(self.filters, self.stride, self.kind != "none")], mfma="fp32", trainable_adjacency=dense)
        assert eng.kinds[0] == self.kind
        return eng

    def forward(self, x, A, training=None):
        _require(x, 4, "x (B, C, T, V)")
        _require(A, 3, "A (K, V, V)")
        B, C, T, V = x.shape
        if tuple(A.shape) != (KS, V, V) or V > 64:
            raise ValueError("A must be (%d, V, V) with V = %d <= 64, got %s" % (KS, V, tuple(A.shape)))
        if training is None:
            training = self.training
        self.build(C, x.device)
        eng = self._engine(A, V, x.device)
        self._calls += 1
        if not training:
            y, To, _ = eng.block_forward(0, to_cn(x), B, T, False)
            return from_cn(y, (B, self.filters, To, V)), A
        return _BlockFunction.apply(x, A, self, eng, *[t for _, t in self._names()]), A


class _TemporalAttentionFn(torch.autograd.Function):
    """TemporalAttention as one node; params = (kernel, bias) per layer"""

    @staticmethod
    def forward(ctx, x, save, *params):
        out, saved = ops.tattn_forward(x, params)
        if save:
            ctx.save_for_backward(x, *saved, *params)
            ctx.nsaved = len(saved)
        a = saved[0]
        ctx.mark_non_differentiable(a)
        return out, a

    @staticmethod
    def backward(ctx, dout, _da):
        x, rest = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        saved, params = rest[:ctx.nsaved], rest[ctx.nsaved:]
        dx, grads = ops.tattn_backward(x, saved, params, dout.contiguous(), need_dx=ctx.needs_input_grad[0])
        return (dx, None) + tuple(grads)


class _Dense(torch.nn.Module):
    """tf.keras.layers.Dense(units)'s variables in the Keras layouts -- kernel (in, units), bias (units) --, created on the first call
    (or by load_state_dict) with the Keras default initialisers: glorot_uniform, zeros"""

    def __init__(self, units):
        super().__init__()
        self.units = int(units)
        self.register_parameter("kernel", None)
        self.register_parameter("bias", None)

    def build(self, in_features, device):
        if self.kernel is None:
            limit = math.sqrt(6.0 / (in_features + self.units))
            kernel = (torch.rand(int(in_features), self.units, dtype=torch.float64) * 2 - 1) * limit
            self.kernel = torch.nn.Parameter(kernel.to(torch.float32).to(device))
            self.bias = torch.nn.Parameter(torch.zeros(self.units, dtype=torch.float32, device=device))
        elif self.kernel.shape[0] != in_features:
            raise ValueError("the layer was built for %d input features, got %d" % (self.kernel.shape[0], in_features))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if self.kernel is None and k is not None:
            self.build(k.shape[0], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class TemporalAttention(torch.nn.Module):
    """models/stgcn.py:67-85; see the module docstring.  forward(x (N, C, T, V), training) -> (N, C, T, V); `training` changes nothing
    (no dropout, no BatchNorm) and is kept for the signature.  Parameters: mlp.{i}.kernel (in, units), mlp.{i}.bias (units), widths
    num_hidden + [1], the first `in` = V C with feature index v C + c.  After a call `last_attention` (N, T) holds the gate (detached).
    Limits (ValueError before anything is built or launched): x a contiguous float32 CUDA tensor, V <= 64, every width <= 128,
    N T < 2^22."""

    def __init__(self, num_hidden):
        super().__init__()
        widths = [int(w) for w in num_hidden] + [1]
        if any(w < 1 or w > ops.TATTN_UMAX for w in widths):
            raise ValueError("the kernels are built for 1 <= units <= %d, got %r" % (ops.TATTN_UMAX, list(num_hidden)))
        self.num_hidden = list(num_hidden)
        self.mlp = torch.nn.ModuleList(_Dense(w) for w in widths)
        self.last_attention = None

    def forward(self, x, training=None):
        _require(x, 4, "x (N, C, T, V)")
        N, C, T, V = x.shape
        if min(N, C, T, V) < 1 or V > ops.TATTN_VMAX:
            raise ValueError("need a non-empty x with V <= %d, got %s" % (ops.TATTN_VMAX, tuple(x.shape)))
        if T * N >= 1 << 22:
            raise ValueError("N T = %d rows: the kernels are built for fewer than 2^22" % (T * N))
        if self.mlp[0].kernel is not None and self.mlp[0].kernel.shape[0] != V * C:
            raise ValueError("the layer was built for %d input features, got V C = %d" % (self.mlp[0].kernel.shape[0], V * C))
        features = V * C
        for layer in self.mlp:
            layer.build(features, x.device)
            features = layer.units
        params = [t for layer in self.mlp for t in (layer.kernel, layer.bias)]
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        out, a = _TemporalAttentionFn.apply(x, save, *params)
        self.last_attention = a.detach().view(N, T)
        return out
