"""A temporal convolution with any kernel size, dilation and stride as a torch module on the HIP kernels (fp32): the temporal unit of the
skeleton models after 2s-AGCN (the MS-TCN branches of MS-G3D, CTR-GCN, InfoGCN and HD-GCN: 3 taps with dilation 1-4, 5 taps with
dilation 1-2, stride 2 in the down-sampling blocks).  The reference's own models use one shape of it, the 9-tap convolution inside
`SpatioTemporalGraphConv`; this module is the operator on its own:

  TemporalConv(filters, kernel_size=9, stride=1, dilation=1, padding="same", use_bias=True)      forward(x (N,C,T,V)) -> (N,filters,T_out,V)

stands for Keras Conv2D(filters, [k, 1], strides=[s, 1], dilation_rate=[d, 1], data_format='channels_first'):

  out[n,m,to,v] = bias[m] + sum_{j<k} sum_c kernel[j,0,c,m] x[n, c, to s + j d - pad, v]          (x is 0 outside [0, T))

padding="same" is TensorFlow's SAME with the dilated extent (T_out = ceil(T / s); the odd frame of padding goes behind), padding=p (an
int) is PyTorch's symmetric padding (sar_amd.ops.tconv_geometry).  One call is ONE autograd node over sar_amd.ops.tconv_forward /
tconv_backward_data / tconv_wgrad (csrc/tconv.hip: three products on the fp32 MFMA pipe that read x and dout where they lie, NCHW, with
no to_cn / from_cn copy); its backward launches only what needs_input_grad asks for -- no data-gradient launch when x needs no gradient,
no weight-gradient launch when neither parameter does.  Parameters `kernel` (k, 1, C, filters) and `bias` (filters) in the Keras layouts,
created on the first call (or by load_state_dict) with VarianceScaling(2, fan_out, truncated_normal) and a zero bias, as every layer of
models/gcn.py.  Under no_grad, or when nothing requires a gradient, nothing is saved.

Limits (ValueError at construction): 1 <= kernel_size <= 9, 1 <= dilation <= 8, stride 1 or 2, 1 <= filters <= 512, an int padding in
[0, (k - 1) d]; (ValueError at the call, before anything is built or launched): a contiguous float32 CUDA x with 1 <= C <= 512,
1 <= V <= 64, N <= 65535 and fewer than 2^31 elements in x and in the result."""
import torch

from models.gcn import _require, variance_scaling_
from sar_amd import ops


class _TemporalConvFn(torch.autograd.Function):
    """the whole layer as one node: gradients for x, kernel and bias, each only where asked for"""

    @staticmethod
    def forward(ctx, x, kernel, bias, geo, save):
        s, d, pad, T_out = geo
        out = ops.tconv_forward(x, kernel, bias, s, d, pad, T_out)
        if save:
            ctx.save_for_backward(x, kernel)
            ctx.geo = geo
        return out

    @staticmethod
    def backward(ctx, dout):
        x, kernel = ctx.saved_tensors
        s, d, pad, _ = ctx.geo
        need_x, need_k, need_b = ctx.needs_input_grad[:3]
        dout = dout.contiguous()
        dx = ops.tconv_backward_data(dout, kernel, x.shape[2], s, d, pad) if need_x else None
        dk, db = ops.tconv_wgrad(x, dout, kernel.shape[0], s, d, pad) if (need_k or need_b) else (None, None)
        return dx, (dk if need_k else None), (db if need_b else None), None, None


class TemporalConv(torch.nn.Module):
    """see the module docstring.  forward(x (N, C, T, V), training=None) -> (N, filters, T_out, V)"""

    def __init__(self, filters, kernel_size=9, stride=1, dilation=1, padding="same", use_bias=True):
        super().__init__()
        self.filters, self.kernel_size, self.stride, self.dilation = int(filters), int(kernel_size), int(stride), int(dilation)
        self.padding, self.use_bias = padding, bool(use_bias)
        if padding != "same" and (isinstance(padding, bool) or not isinstance(padding, int)):
            raise ValueError("padding must be \"same\" or a number of frames (got %r)" % (padding,))
        ops.tconv_limits(self.kernel_size, self.dilation, self.stride, 0 if padding == "same" else padding, M=self.filters)
        self.register_parameter("kernel", None)
        self.register_parameter("bias", None)

    def build(self, in_channels, device):
        if self.kernel is None:
            self.kernel = torch.nn.Parameter(torch.empty((self.kernel_size, 1, int(in_channels), self.filters), dtype=torch.float32, device=device))
            variance_scaling_(self.kernel)
            if self.use_bias:
                self.bias = torch.nn.Parameter(torch.zeros(self.filters, dtype=torch.float32, device=device))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if self.kernel is None and k is not None:
            self.build(k.shape[-2], k.device if k.is_cuda else "cuda")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def check(self, x):
        """every limit of the call: ValueError before a parameter is built or a kernel launched -> (T_out, pad)"""
        _require(x, 4, "x (N, C, T, V)")
        N, C, T, V = x.shape
        if min(N, C, T, V) < 1:
            raise ValueError("need a non-empty x, got %s" % (tuple(x.shape),))
        T_out, pad = ops.tconv_geometry(T, self.kernel_size, self.stride, self.dilation, self.padding)
        ops.tconv_limits(self.kernel_size, self.dilation, self.stride, pad, C, self.filters, V, N)
        if x.numel() >= 1 << 31 or N * self.filters * T_out * V >= 1 << 31:
            raise ValueError("TemporalConv is built for fewer than 2^31 elements per tensor (got x %s, filters = %d)" % (tuple(x.shape), self.filters))
        if self.kernel is not None and self.kernel.shape[2] != C:
            raise ValueError("the layer was built for %d input channels, got %d" % (self.kernel.shape[2], C))
        return T_out, pad

    def forward(self, x, training=None):
        T_out, pad = self.check(x)
        self.build(x.shape[1], x.device)
        ts = (x, self.kernel) + ((self.bias,) if self.use_bias else ())
        save = torch.is_grad_enabled() and any(t.requires_grad for t in ts)
        return _TemporalConvFn.apply(x, self.kernel, self.bias if self.use_bias else None, (self.stride, self.dilation, pad, T_out), save)
