"""CPU: the ABI of csrc/tattn.hip (include/sar_hip.h, TemporalAttention).  Every sar_tattn_* prototype of the header has a row of
matching arity in sar_amd/_lib.py; the entry points check pointers, sizes and strides before anything is launched, so they answer on
a machine without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()); the wrappers of
sar_amd/ops.py and the module models.stgcn.TemporalAttention reject what the kernels are not built for before they touch the library."""
import ctypes
import os
import re

import pytest
import torch

from sar_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototypes():
    hdr = open(os.path.join(ROOT, "include", "sar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_tattn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_every_prototype_has_a_binding_row_of_matching_arity():
    protos = _prototypes()
    assert len(protos) == 8 and {"sar_tattn_score_f32", "sar_tattn_scale_f32", "sar_tattn_dscore_f32", "sar_tattn_wgrad_f32",
                                 "sar_tattn_dx_f32"} <= set(protos)
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_tattn_")}
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
UNITS = ("sar_tattn_score_f32", "sar_tattn_wgrad_f32", "sar_tattn_dx_f32")          # take units and a [units][ld] matrix
RELU, SIGMOID = 0, 1


def _calls(lib, p, N, C, T, V, u, sn=None, sc=None, ld=None, act=RELU, nslab=None):
    """the five kernels of the layer with the same sizes; p = what stands in for each pointer; (sn, sc) default to NCHW, ld to N T"""
    sn, sc = (C * T * V, T * V) if sn is None else (sn, sc)
    ld = N * T if ld is None else ld
    q = None if p is None else p + 32           # dx may not be dout
    if nslab is None:
        nslab = max(lib.sar_tattn_wgrad_slabs(N, C, T, V), 1)
    return [
        ("sar_tattn_score_f32", lambda: lib.sar_tattn_score_f32(p, sn, sc, p, p, N, C, T, V, u, act, p, ld, None)),
        ("sar_tattn_scale_f32", lambda: lib.sar_tattn_scale_f32(p, sn, sc, p, N, C, T, V, p, sn, sc, None)),
        ("sar_tattn_dscore_f32", lambda: lib.sar_tattn_dscore_f32(p, sn, sc, p, sn, sc, p, N, C, T, V, p, None)),
        ("sar_tattn_wgrad_f32", lambda: lib.sar_tattn_wgrad_f32(p, sn, sc, p, ld, N, C, T, V, u, p, nslab, None)),
        ("sar_tattn_dx_f32", lambda: lib.sar_tattn_dx_f32(p, sn, sc, p, p, p, ld, N, C, T, V, u, q, sn, sc, None)),
    ]


def test_null_operands_are_argument_errors(lib):
    for name, call in _calls(lib, None, 2, 4, 3, 5, 6):
        _rejected(lib, call(), ARG, name)
    _rejected(lib, lib.sar_tattn_act_f32(None, 8, 2, 8, RELU, None), ARG, "sar_tattn_act_f32")
    _rejected(lib, lib.sar_tattn_dact_f32(None, 8, None, 8, 2, 8, None), ARG, "sar_tattn_dact_f32")


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 129):                   # units = 129
        if name in UNITS:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 0):                     # units = 0
        if name in UNITS:
            _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 4, 3, 65, 6, nslab=1):           # V = 65
        _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 4, 3, 0, 6, nslab=1):            # V = 0
        _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 0, 3, 5, 6, nslab=1):            # C = 0
        _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 1 << 12, 1, 1 << 10, 1, 6, nslab=1):     # N T = 2^22
        _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 1 << 11, 1 << 9, 1 << 10, 2, 6, nslab=1):     # 2^31 elements, N T = 2^21
        _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 6, ld=5):               # a [units][ld] matrix with ld < N T
        if name in UNITS:
            _rejected(lib, call(), ARG, name)
    for sn, sc in ((4 * 3 * 5, 3 * 5 - 1), (3 * 5 - 1, 2 * 3 * 5), (3 * 5, 2 * 3 * 5 - 1), (4 * 3 * 5 - 1, 3 * 5), (0, 15), (60, -15)):
        for name, call in _calls(lib, p, 2, 4, 3, 5, 6, sn, sc):         # runs that overlap or run backwards
            _rejected(lib, call(), ARG, name)
    _rejected(lib, lib.sar_tattn_score_f32(p, 60, 15, p, p, 2, 4, 3, 5, 6, 2, p, 6, None), ARG, "sar_tattn_score_f32")      # act = 2
    _rejected(lib, lib.sar_tattn_wgrad_f32(p, 60, 15, p, 6, 2, 4, 3, 5, 6, p, 7, None), ARG, "sar_tattn_wgrad_f32")         # not the slab count
    _rejected(lib, lib.sar_tattn_dx_f32(p, 60, 15, p, p, p, 6, 2, 4, 3, 5, 6, p, 60, 15, None), ARG, "sar_tattn_dx_f32")    # dx is dout
    _rejected(lib, lib.sar_tattn_act_f32(p, 7, 2, 8, RELU, None), ARG, "sar_tattn_act_f32")                                # ld < n
    _rejected(lib, lib.sar_tattn_act_f32(p, 8, 129, 8, RELU, None), ARG, "sar_tattn_act_f32")
    _rejected(lib, lib.sar_tattn_act_f32(p, 8, 2, 8, 2, None), ARG, "sar_tattn_act_f32")
    _rejected(lib, lib.sar_tattn_dact_f32(p, 8, p, 7, 2, 8, None), ARG, "sar_tattn_dact_f32")
    # the slab count is a function of the shape alone
    assert lib.sar_tattn_wgrad_slabs(128, 64, 300, 25) == 32 and lib.sar_tattn_wgrad_slabs(128, 256, 75, 25) == 8
    assert lib.sar_tattn_wgrad_slabs(2, 16, 300, 25) == 5 and lib.sar_tattn_wgrad_slabs(1, 3, 1, 25) == 1
    assert lib.sar_tattn_wgrad_slabs(0, 3, 1, 25) == _lib.SAR_E_ARG and lib.sar_tattn_wgrad_slabs(2, 3, 1, 65) == _lib.SAR_E_UNSUP


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    N, C, T, V = 2, 4, 3, 5
    x = _f(N, C, T, V)
    params = [_f(V * C, 6), _f(6), _f(6, 1), _f(1)]
    with pytest.raises(ValueError, match="CUDA"):                        # host tensors
        ops.tattn_forward(x, params)
    with pytest.raises(ValueError, match="V <= 64"):
        ops.tattn_forward(_f(N, C, T, 65), [_f(65 * C, 1), _f(1)])
    with pytest.raises(ValueError, match="units <= 128"):
        ops.tattn_forward(x, [_f(V * C, 129), _f(129), _f(129, 1), _f(1)])
    with pytest.raises(ValueError, match="2\\^22"):
        ops.tattn_forward(_f(1 << 12, 1, 1 << 10, 1), [_f(1, 1), _f(1)])
    with pytest.raises(ValueError, match="one unit"):                    # no closing Dense(1)
        ops.tattn_forward(x, params[:2])
    with pytest.raises(ValueError, match="layer 0"):                     # a kernel for other features
        ops.tattn_forward(x, [_f(V * C + 1, 1), _f(1)])
    with pytest.raises(ValueError, match="layer 1"):                     # widths that do not chain
        ops.tattn_forward(x, [_f(V * C, 6), _f(6), _f(5, 1), _f(1)])
    with pytest.raises(ValueError, match="4-D"):
        ops.tattn_forward(_f(N, C, T * V), params)
    with pytest.raises(ValueError, match="float32"):
        ops.tattn_forward(x.double(), params)
    with pytest.raises(ValueError, match="inner strides"):               # a vertex stride
        ops.tattn_forward(_f(N, C, T, 2 * V)[..., ::2], params)
    with pytest.raises(ValueError, match="inner strides"):               # frame-major: neither NCHW nor CN
        ops.tattn_forward(_f(T, N, C, V).permute(1, 2, 0, 3), params)
    saved = (_f(N * T), _f(6, N * T))
    with pytest.raises(ValueError, match="CUDA"):
        ops.tattn_backward(x, saved, params, _f(N, C, T, V))
    with pytest.raises(ValueError, match="shape"):                       # dout of another shape
        ops.tattn_backward(x, saved, params, _f(N, C, T + 1, V))
    with pytest.raises(ValueError, match="saved"):
        ops.tattn_backward(x, saved[:1], params, _f(N, C, T, V))


def test_module_rejects_without_building_or_launching(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    from models.stgcn import TemporalAttention
    with pytest.raises(ValueError, match="units <= 128"):
        TemporalAttention([129])
    with pytest.raises(ValueError, match="units <= 128"):
        TemporalAttention([0])
    m = TemporalAttention([6])
    assert [n for n, _ in m.named_parameters()] == [] and m.num_hidden == [6] and m.last_attention is None
    for bad in (_f(2, 4, 3, 5), _f(2, 4, 15)):                           # a host tensor, three dimensions
        with pytest.raises(ValueError, match="contiguous float32 CUDA"):
            m(bad, True)
    assert [n for n, _ in m.named_parameters()] == [], "a rejected call built the parameters"
