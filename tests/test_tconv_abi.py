"""CPU: the ABI of csrc/tconv.hip (include/sar_hip.h, TemporalConv).  Every sar_tconv_* prototype of the header has a row of matching
arity and types in sar_amd/_lib.py; the entry points check pointers, sizes and strides before anything is launched, so they answer on a
machine without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()); the wrappers of sar_amd/ops.py and
models.tcn.TemporalConv reject what the kernels are not built for before they touch the library."""
import ctypes
import os
import re

import pytest
import torch

from sar_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("sar_tconv_fwd_f32", "sar_tconv_bwd_data_f32", "sar_tconv_wgrad_f32")


def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "sar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_tconv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_every_prototype_has_a_binding_row_of_matching_arity_and_types():
    protos = _prototypes()
    assert set(protos) == set(KERNELS) | {"sar_tconv_wgrad_slabs"}
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_tconv_")}
    for name, args in protos.items():
        params = [a.strip() for a in args.split(",") if a.strip()]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for a, ty in zip(params, argtypes):          # pointers cross as void*, int64_t as c_int64, int as c_int
            want = ctypes.c_void_p if ("*" in a or "sar_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
            assert ty is want, (name, a, ty)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _rejected(lib, rc, want, name):
    assert rc in want, "%s returned %d, expected one of %s" % (name, rc, want)
    assert name.encode() in lib.sar_last_error_string()


ARG, UNSUP = (_lib.SAR_E_ARG,), (_lib.SAR_E_UNSUP,)
GOOD = dict(N=2, C=3, M=4, T=6, T_out=6, V=5, k=3, d=2, s=1, pad=2)


def _calls(lib, p, x_strides=None, o_strides=None, nslab=1, **over):
    """the three kernels with the same sizes; p = the base of what stands in for the pointers (distinct operands 64 bytes apart);
    the strides default to NCHW"""
    g = dict(GOOD, **over)
    N, C, M, T, T_out, V, k, d, s, pad = (g[n] for n in ("N", "C", "M", "T", "T_out", "V", "k", "d", "s", "pad"))
    xn, xc = (C * T * V, T * V) if x_strides is None else x_strides
    on, oc = (M * T_out * V, T_out * V) if o_strides is None else o_strides
    q = [None] * 4 if p is None else [p + 64 * i for i in range(4)]
    return [
        ("sar_tconv_fwd_f32", lambda: lib.sar_tconv_fwd_f32(q[0], xn, xc, q[1], q[2], N, C, M, T, T_out, V, k, d, s, pad, q[3], on, oc, None)),
        ("sar_tconv_bwd_data_f32", lambda: lib.sar_tconv_bwd_data_f32(q[0], on, oc, q[1], N, C, M, T, T_out, V, k, d, s, pad, q[3], xn, xc, None)),
        ("sar_tconv_wgrad_f32", lambda: lib.sar_tconv_wgrad_f32(q[0], xn, xc, q[1], on, oc, N, C, M, T, T_out, V, k, d, s, pad, q[3], nslab, None)),
    ]


def test_null_operands_are_argument_errors(lib):
    for name, call in _calls(lib, None):
        _rejected(lib, call(), ARG, name)


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 128)()
    p = ctypes.addressof(buf)
    for over in (dict(k=10, pad=0), dict(d=9), dict(s=3), dict(V=65), dict(C=513), dict(M=513), dict(pad=5), dict(k=1, pad=1), dict(N=65536),
                 dict(N=4096, C=512, T=1024, T_out=1024, V=1)):                                   # 2^31 elements
        for name, call in _calls(lib, p, **over):
            _rejected(lib, call(), UNSUP, name)
    for over in (dict(N=0), dict(C=0), dict(M=0), dict(T=0), dict(T_out=0), dict(V=0), dict(k=0), dict(d=0), dict(s=0), dict(pad=-1),
                 dict(T_out=8),                                # the last window would start behind the last frame and its padding
                 dict(T=4, T_out=6)):
        for name, call in _calls(lib, p, **over):
            _rejected(lib, call(), ARG, name)
    # an ld shorter than its row: NCHW channel stride T V - 1, a CN matrix whose ld is N T V - 1, a sample stride of 0
    for kw in (dict(x_strides=(3 * 30, 29)), dict(x_strides=(30, 59)), dict(x_strides=(0, 30)), dict(o_strides=(4 * 30, 29)),
               dict(o_strides=(30, 59)), dict(o_strides=(30, 1 << 31))):
        for name, call in _calls(lib, p, **kw):
            _rejected(lib, call(), ARG, name)
    # an output that is an input
    a, b, c = p, p + 64, p + 128
    N, C, M, T, V = 2, 3, 4, 6, 5
    xs, os_ = (C * T * V, T * V), (M * T * V, T * V)
    for out in (a, b, c):
        _rejected(lib, lib.sar_tconv_fwd_f32(a, *xs, b, c, N, C, M, T, T, V, 3, 2, 1, 2, out, *os_, None), ARG, "sar_tconv_fwd_f32")
    for out in (a, b):
        _rejected(lib, lib.sar_tconv_bwd_data_f32(a, *os_, b, N, C, M, T, T, V, 3, 2, 1, 2, out, *xs, None), ARG, "sar_tconv_bwd_data_f32")
        _rejected(lib, lib.sar_tconv_wgrad_f32(a, *xs, b, *os_, N, C, M, T, T, V, 3, 2, 1, 2, out, 1, None), ARG, "sar_tconv_wgrad_f32")
    _rejected(lib, lib.sar_tconv_wgrad_f32(a, *xs, b, *os_, N, C, M, T, T, V, 3, 2, 1, 2, c, 2, None), ARG, "sar_tconv_wgrad_f32")   # not the slab count


def test_slab_count_is_a_function_of_the_shape_alone(lib):
    """about 512 workgroups of (32 channels, 64 filters), at least 4 tiles of 64 columns of one sample to a slab, at most 256 slabs;
    k, d, s and pad are not even arguments"""
    slabs = lib.sar_tconv_wgrad_slabs
    assert slabs(1, 1, 1, 1, 1) == 1 and slabs(4, 1, 1, 1, 1) == 1 and slabs(4, 64, 64, 2, 25) == 1       # 4 tiles: still one
    assert slabs(5, 1, 1, 1, 1) == 2 and slabs(5, 3, 2, 4, 5) == 2                                         # 5 tiles: the first size with two
    assert slabs(1, 8, 8, 13, 5) == 1 and slabs(1, 8, 8, 52, 5) == 2                                       # 260 columns of one sample: 5 tiles
    assert slabs(2, 64, 64, 13, 25) == 3                                                                   # 12 tiles
    assert slabs(128, 64, 64, 300, 25) == 256 and slabs(128, 16, 16, 300, 25) == 256                       # the workload: the cap
    assert slabs(128, 256, 256, 75, 25) == 16 and slabs(128, 512, 512, 75, 25) == 4                        # 32 / 128 blocks of the kernel
    assert slabs(0, 3, 3, 3, 25) == _lib.SAR_E_ARG and slabs(2, 3, 3, 3, 65) == _lib.SAR_E_UNSUP and slabs(2, 513, 3, 3, 25) == _lib.SAR_E_UNSUP
    assert b"sar_tconv_wgrad_slabs" in lib.sar_last_error_string()


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    _no_library(monkeypatch)
    N, C, M, T, V, k = 2, 3, 4, 6, 5, 3
    x, W, b, dout = _f(N, C, T, V), _f(k, 1, C, M), _f(M), _f(N, M, T, V)
    fwd, bwd, wg = ops.tconv_forward, ops.tconv_backward_data, ops.tconv_wgrad
    with pytest.raises(ValueError, match="CUDA"):                        # host tensors
        fwd(x, W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="CUDA"):
        bwd(dout, W, T, 1, 2, 2)
    with pytest.raises(ValueError, match="CUDA"):
        wg(x, dout, k, 1, 2, 2)
    with pytest.raises(ValueError, match="float32"):
        fwd(x.double(), W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="4-D"):
        fwd(_f(N, C, T * V), W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="inner strides"):               # a joint stride
        fwd(_f(N, C, T, 2 * V)[..., ::2], W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="inner strides"):               # channels-last
        fwd(_f(N, T, V, C).permute(0, 3, 1, 2), W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="Keras kernel"):                # a kernel for other channels
        fwd(x, _f(k, 1, C + 1, M), b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="Keras kernel"):
        fwd(x, _f(k, C, M), b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="contiguous"):
        fwd(x, _f(k, 1, C, 2 * M)[..., ::2], b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="bias"):
        fwd(x, W, _f(M + 1), 1, 2, 2, T)
    with pytest.raises(ValueError, match="out must"):
        fwd(x, W, b, 1, 2, 2, T, out=_f(N, M, T + 1, V))
    for bad in (dict(stride=3), dict(dilation=9), dict(pad=5), dict(dilation=0), dict(stride=0), dict(pad=-1)):
        g = dict(dict(stride=1, dilation=2, pad=2), **bad)
        with pytest.raises(ValueError, match="built for"):
            fwd(x, W, b, g["stride"], g["dilation"], g["pad"], T)
        with pytest.raises(ValueError, match="built for"):
            bwd(dout, W, T, g["stride"], g["dilation"], g["pad"])
        with pytest.raises(ValueError, match="built for"):
            wg(x, dout, k, g["stride"], g["dilation"], g["pad"])
    with pytest.raises(ValueError, match="built for"):                   # k = 10
        fwd(x, _f(10, 1, C, M), b, 1, 1, 0, T)
    with pytest.raises(ValueError, match="built for"):
        wg(x, dout, 10, 1, 1, 0)
    with pytest.raises(ValueError, match="built for"):                   # V = 65
        fwd(_f(N, C, T, 65), W, b, 1, 2, 2, T)
    with pytest.raises(ValueError, match="built for"):                   # C = 513
        fwd(_f(1, 513, 2, 2), _f(1, 1, 513, M), b, 1, 1, 0, 2)
    with pytest.raises(ValueError, match="built for"):                   # 513 filters
        fwd(x, _f(k, 1, C, 513), None, 1, 2, 2, T)
    with pytest.raises(ValueError, match="reads past"):                  # a T_out the padding does not reach
        fwd(x, W, b, 1, 2, 2, T + 2)
    with pytest.raises(ValueError, match="reads past"):
        bwd(_f(N, M, T + 2, V), W, T, 1, 2, 2)
    with pytest.raises(ValueError, match="filters"):                     # dout of another width than the kernel
        bwd(_f(N, M + 1, T, V), W, T, 1, 2, 2)
    with pytest.raises(ValueError, match="dout must"):                   # dout of another batch than x
        wg(x, _f(N + 1, M, T, V), k, 1, 2, 2)
    with pytest.raises(ValueError, match="dx must"):
        bwd(dout, W, T, 1, 2, 2, dx=_f(N, C, T + 1, V))


def test_module_rejects_without_building_or_launching(monkeypatch):
    _no_library(monkeypatch)
    from models.tcn import TemporalConv
    for bad in (dict(kernel_size=10), dict(kernel_size=0), dict(dilation=9), dict(dilation=0), dict(stride=3), dict(stride=0), dict(filters=513),
                dict(filters=0), dict(kernel_size=3, dilation=2, padding=5), dict(padding=-1), dict(padding="valid"), dict(padding=1.5),
                dict(kernel_size=1, padding=1)):
        with pytest.raises(ValueError):
            TemporalConv(**dict(dict(filters=8), **bad))
    m = TemporalConv(8, 5, stride=2, dilation=2)
    assert (m.filters, m.kernel_size, m.stride, m.dilation, m.padding, m.use_bias) == (8, 5, 2, 2, "same", True)
    assert TemporalConv(8).kernel_size == 9 and TemporalConv(8, 3, padding=2, dilation=2, use_bias=False).padding == 2
    assert [n for n, _ in m.named_parameters()] == []
    for x in (_f(2, 4, 6, 5), _f(2, 4, 30), _f(2, 4, 6, 5).double(), _f(2, 4, 6, 10)[..., ::2]):      # host, 3-D, float64, strided
        with pytest.raises(ValueError, match="contiguous float32 CUDA"):
            m(x)
    assert [n for n, _ in m.named_parameters()] == [], "a rejected call built the parameters"
