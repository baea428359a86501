"""The operand checks of the layer wrappers (sar_amd/ops.py: pgc_*, pgpool_*, gpool_*, tattn_*, adjattn_*), written once.  Each takes
`what` (the operand's name) or `layer` for the message and raises ValueError; none touches the library.  The size limits of a layer
stay with the layer."""
import torch


def _got(t):
    return "shape %s, strides %s" % (tuple(t.shape), tuple(t.stride())) if torch.is_tensor(t) else type(t).__name__


def on_gpu(layer, f32=(), i32=()):
    """every operand of f32 is a float32 CUDA tensor, every operand of i32 an int32 one"""
    for ts, dtype, name in ((f32, torch.float32, "float32"), (i32, torch.int32, "int32")):
        for t in ts:
            if not (torch.is_tensor(t) and t.dtype == dtype and t.is_cuda):
                raise ValueError("%s operands must be %s CUDA tensors (got %s)" % (
                    layer, name, ("%s on %s" % (t.dtype, t.device)) if torch.is_tensor(t) else type(t).__name__))


def cn_matrix(t, rows, cols, what):
    """a CN matrix [rows][cols] (rows=None: any number >= 1), contiguous or a row-strided view -> its leading dimension"""
    if not (torch.is_tensor(t) and t.dim() == 2 and (t.shape[0] >= 1 if rows is None else t.shape[0] == rows) and t.shape[1] == cols
            and t.stride(1) == 1 and t.stride(0) >= cols):
        raise ValueError("%s must be a CN matrix: a 2-D tensor of %s rows and %d columns, contiguous or a row-strided view with a unit "
                         "column stride (got %s)" % (what, "C" if rows is None else rows, cols, _got(t)))
    return t.stride(0)


def dense(t, shape, what):
    """a contiguous tensor of `shape` (None: of any shape)"""
    if not (torch.is_tensor(t) and (shape is None or tuple(t.shape) == tuple(shape)) and t.is_contiguous()):
        raise ValueError("%s must be a contiguous tensor%s (got %s)" % (what, "" if shape is None else " of shape %s" % (tuple(shape),), _got(t)))


def view4(t, shape, what):
    """a 4-D (N, C, T, W) tensor or view of `shape` whose two inner strides are (W, 1), channel-major per sample (NCHW) or sample-major
    per channel (the view X[:, :N*T*W].view(C, N, T, W).permute(1, 0, 2, 3) of a CN matrix) -> (sample stride, channel stride)"""
    if not (torch.is_tensor(t) and t.dim() == 4 and tuple(t.shape) == tuple(shape)):
        raise ValueError("%s must be a 4-D tensor of shape %s (got %s)" % (what, tuple(shape), _got(t)))
    N, C, T, W = shape
    sn, sc = t.stride(0), t.stride(1)
    inner = (T == 1 or t.stride(2) == W) and (W == 1 or t.stride(3) == 1)
    nchw = sc >= T * W and (C == 1 or N == 1 or sn >= C * sc)
    cn = sn >= T * W and (N == 1 or C == 1 or sc >= N * sn)
    if not (inner and (nchw or cn)):
        raise ValueError("%s must have unit inner strides (W, 1) and be channel-major per sample (NCHW) or sample-major per channel (a CN "
                         "matrix): got %s" % (what, _got(t)))
    return sn, sc
