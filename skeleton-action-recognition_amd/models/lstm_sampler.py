"""Drop-in for the reference's models/lstm_sampler.py: `TemporalSampler`, the frame sampler that sits in front of a graph network,
as a torch module whose arithmetic runs in libsar_hip.so (fp32, csrc/lstm.hip).

  TemporalSampler(num_hidden, top_k=200)      forward(x (N,C,T,V), training) -> (N,C,top_k,V)      models/lstm_sampler.py:1-27

What it computes (Keras / TF2 defaults restated):
  * x_lstm[n, t, v C + c] = x[n, c, t, v]; a stack of LSTM layers of widths num_hidden + [1], each return_sequences=True with zero
    initial state, gate order i, f, c, o along the 4u axis, tanh / sigmoid, with bias:
        z_t = x_t kernel + h_{t-1} recurrent_kernel + bias;  i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_c)
        c_t = f c_{t-1} + i g;  h_t = o tanh(c_t)
  * the scores are the last layer's h, ALWAYS taken as (N, T).  The reference's bare tf.squeeze would also drop a batch of N = 1
    (and then fail in top_k / gather); that is not copied.
  * values, indices = top_k(scores, k=top_k, sorted=False).  TF leaves the order open for sorted=False; this port FIXES it:
    DESCENDING by score, equal scores in ASCENDING frame index -- TF's documented tie rule and one of the orders TF may return.
    The next layer is a temporal convolution, so the order of the gathered frames is part of the result.
  * out[n, c, j, v] = x[n, c, idx[n, j], v] * values[n, j]: the scorer trains through the scale.
  * `training` changes nothing (the reference's LSTMs have no dropout); it is kept for the signature.

Parameters keep the Keras layouts and names -- `lstm_model.{i}.kernel` (F, 4u), `lstm_model.{i}.recurrent_kernel` (u, 4u),
`lstm_model.{i}.bias` (4u) -- are created on the first call as Keras' `build` does (or by load_state_dict), and are initialised with
the Keras defaults: glorot_uniform, orthogonal, zeros with the forget quarter at one (unit_forget_bias).

The whole call is ONE torch.autograd.Function over sar_amd.ops:
  * sar_lstm_pack_f32 lays x out as the stack's input matrix [V C][T N] with TIME-MAJOR columns t N + n;
  * per layer, zin = kernel^T X + bias over all T N columns at once is the layers' 1x1 product (ops.conv1x1_fwd), and
    sar_lstm_fwd_f32 walks the T steps in one launch (recurrent weights resident on chip);
  * sar_topk_desc_f32, sar_frame_gather_f32;
  * backward: sar_frame_gather_bwd_f32 (dvalues, the scattered dscores, the gather path's dx), then per layer from the top
    sar_lstm_bwd_f32 (dz), (d kernel, d bias) = conv1x1_wgrad(X, dz), d recurrent_kernel = sum_t h_{t-1} dz_t^T as the same launch on
    the VIEWS h[:, 0 : (T-1) N] and dz[:, N : T N] (time-major columns: h_{t-1} is h shifted by N columns), dX = kernel dz
    (conv1x1_dgrad); the first layer's dX only when x requires a gradient, added into dx by sar_lstm_unpack_add_f32.
Indices carry no gradient.  Under torch.no_grad(), or when nothing requires a gradient, the kernels get NULL save pointers
(the gates and c are not written).

Limits (ValueError before any launch): x a contiguous float32 CUDA (N, C, T, V) tensor, top_k <= T <= 2048, every width <= 128,
T N < 2^22 (the 1x1 products' column limit).

Not wired into main_gnn.py (the reference wires it into no model).  In front of a whole-network model (models.stgcn.Model and its
siblings) the scorer trains: the engines return d loss / d clip (INTEGRATION.md has the example)."""
import math

import torch

from models.gcn import _require
from sar_amd import ops

MAX_UNITS, MAX_T = 128, 2048


def _new(rows, cols, dev, dtype=torch.float32):
    return torch.empty((rows, cols), dtype=dtype, device=dev)


class _TemporalSamplerFn(torch.autograd.Function):
    """TemporalSampler as one node; params = (kernel, recurrent_kernel, bias) per layer.  Everything backward needs is kept in ctx."""

    @staticmethod
    def forward(ctx, x, top_k, save, *params):
        N, C, T, V = x.shape
        n, dev, nl = T * N, x.device, len(params) // 3
        geo = ops.column_geometry(T, N)
        X = _new(V * C, n, dev)
        ops.lstm_pack(x, X)
        src, layers = X, []
        for i in range(nl):
            kernel, U, bias = params[3 * i:3 * i + 3]
            u = U.shape[0]
            zin = ops.conv1x1_fwd(src, kernel, bias, geo)
            h = _new(u, n, dev)
            gates, c = (_new(4 * u, n, dev), _new(u, n, dev)) if save else (None, None)
            ops.lstm_fwd(zin, U, h, u, N, T, gates, c)
            layers.append((src, gates, c, h))
            src = h
        values = _new(N, top_k, dev)
        idx, inv = _new(N, top_k, dev, torch.int32), _new(N, T, dev, torch.int32)
        ops.topk_desc(src, 1, N, N, T, top_k, values, idx, inv)          # scores[n, t] = h[0][t N + n]
        out = torch.empty((N, C, top_k, V), dtype=torch.float32, device=dev)
        ops.frame_gather(x, idx, values, out)
        if save:
            ctx.save_for_backward(x, values, *params)
            ctx.idx, ctx.inv, ctx.layers, ctx.geo = idx, inv, layers, geo
        ctx.mark_non_differentiable(idx, src)
        return out, idx, src

    @staticmethod
    def backward(ctx, dout, _didx, _dscores):
        x, values = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        N, C, T, V = x.shape
        n, dev, nl, top_k = T * N, x.device, len(params) // 3, values.shape[1]
        need_x = ctx.needs_input_grad[0]
        dx = torch.empty_like(x) if need_x else None
        dvalues, dh = _new(N, top_k, dev), _new(1, n, dev)
        ops.frame_gather_bwd(x, dout.contiguous(), values, ctx.inv, dvalues, dh, 1, N, dx)
        grads = [None] * len(params)
        for i in range(nl - 1, -1, -1):
            kernel, U, _ = params[3 * i:3 * i + 3]
            src, gates, c, h = ctx.layers[i]
            u = U.shape[0]
            dz = _new(4 * u, n, dev)
            ops.lstm_bwd(dh, gates, c, U, dz, u, N, T)
            grads[3 * i], grads[3 * i + 2] = ops.conv1x1_wgrad(src, dz, ctx.geo)
            grads[3 * i] = grads[3 * i].view(kernel.shape)
            if T > 1:       # sum_t h_{t-1} dz_t^T: h shifted by one step is h shifted by N columns; the launch's bias output is discarded
                grads[3 * i + 1] = ops.conv1x1_wgrad(h[:, :n - N], dz[:, N:], ops.column_geometry(T - 1, N))[0].view(U.shape)
            else:
                grads[3 * i + 1] = torch.zeros_like(U)
            if i > 0:
                dh = ops.conv1x1_dgrad(dz, kernel, ctx.geo)
            elif need_x:
                ops.lstm_unpack_add(ops.conv1x1_dgrad(dz, kernel, ctx.geo), dx)
        return (dx, None, None) + tuple(grads)


class _LSTMLayer(torch.nn.Module):
    """tf.keras.layers.LSTM(units, return_sequences=True)'s variables in the Keras layouts, created on the first call (or by
    load_state_dict) with the Keras default initialisers"""

    def __init__(self, units):
        super().__init__()
        self.units = int(units)
        for name in ("kernel", "recurrent_kernel", "bias"):
            self.register_parameter(name, None)

    def build(self, in_features, device):
        u = self.units
        if self.kernel is None:
            limit = math.sqrt(6.0 / (in_features + 4 * u))                                   # glorot_uniform
            kernel = (torch.rand(int(in_features), 4 * u, dtype=torch.float64) * 2 - 1) * limit
            q, r = torch.linalg.qr(torch.randn(4 * u, u, dtype=torch.float64))              # orthogonal: rows of (u, 4u) orthonormal
            q = q * torch.sign(torch.diagonal(r))
            bias = torch.zeros(4 * u)
            bias[u:2 * u] = 1.0                                                              # unit_forget_bias
            self.kernel = torch.nn.Parameter(kernel.to(torch.float32).to(device))
            self.recurrent_kernel = torch.nn.Parameter(q.t().contiguous().to(torch.float32).to(device))
            self.bias = torch.nn.Parameter(bias.to(device))
        elif self.kernel.shape[0] != in_features:
            raise ValueError("the layer was built for %d input features, got %d" % (self.kernel.shape[0], in_features))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if self.kernel is None and k is not None:
            self.build(k.shape[0], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class TemporalSampler(torch.nn.Module):
    """models/lstm_sampler.py:1-27; see the module docstring.  After a call, `last_indices` (N, top_k) int32 holds the chosen frames in
    output order and `last_scores` (N, T) the scores they were chosen by (detached)."""

    def __init__(self, num_hidden, top_k=200):
        super().__init__()
        widths = [int(w) for w in num_hidden] + [1]
        if not isinstance(top_k, int) or top_k < 1:
            raise ValueError("top_k must be a positive int, got %r" % (top_k,))
        if any(w < 1 or w > MAX_UNITS for w in widths):
            raise ValueError("the LSTM kernels are built for 1 <= units <= %d, got %r" % (MAX_UNITS, list(num_hidden)))
        self.num_hidden, self.top_k = list(num_hidden), top_k
        self.lstm_model = torch.nn.ModuleList(_LSTMLayer(w) for w in widths)
        self.last_indices = self.last_scores = None

    def forward(self, x, training=None):
        _require(x, 4, "x (N, C, T, V)")
        N, C, T, V = x.shape
        if min(N, C, T, V) < 1 or T > MAX_T or self.top_k > T:
            raise ValueError("need 1 <= top_k <= T <= %d and a non-empty x, got top_k = %d, x %s" % (MAX_T, self.top_k, tuple(x.shape)))
        if T * N >= 1 << 22:
            raise ValueError("T N = %d columns: the 1x1 products are built for fewer than 2^22" % (T * N))
        features = V * C
        for layer in self.lstm_model:
            layer.build(features, x.device)
            features = layer.units
        params = [t for layer in self.lstm_model for t in (layer.kernel, layer.recurrent_kernel, layer.bias)]
        save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        out, idx, scores = _TemporalSamplerFn.apply(x, self.top_k, save, *params)
        self.last_indices, self.last_scores = idx, scores.detach().view(T, N).t()
        return out
