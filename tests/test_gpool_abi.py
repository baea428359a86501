"""CPU: the ABI of csrc/gpool.hip (include/sar_hip.h, GPool).  Every sar_gpool_* prototype of the header has a row of matching arity
in sar_amd/_lib.py; the entry points check pointers, sizes and strides before anything is launched, so they answer on a machine
without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()); the wrappers of sar_amd/ops.py
reject what the kernels are not built for before they touch the library."""
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
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_gpool_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_every_prototype_has_a_binding_row_of_matching_arity():
    protos = _prototypes()
    assert len(protos) == 11 and "sar_gpool_score_f32" in protos and "sar_gpool_dp_f32" in protos
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_gpool_")}
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
EITHER = ARG + UNSUP
WALKS = ("sar_gpool_score_f32", "sar_gpool_gather_f32", "sar_gpool_ds_f32", "sar_gpool_dx_f32")          # take strides
ADJ = ("sar_gpool_adj_f32", "sar_gpool_adj_bwd_f32")                                                      # take K, no C / T
NO_SHAPE = ("sar_gpool_prep_f32", "sar_gpool_dp_f32")                                                     # take C T only


def _calls(lib, p, N, C, T, V, K, keep, sn=None, sc=None):
    """every entry point with the same sizes; p = what stands in for each pointer; (sn, sc) default to NCHW"""
    sn_x, sc_x = (C * T * V, T * V) if sn is None else (sn, sc)
    sn_o, sc_o = (C * T * keep, T * keep) if sn is None else (sn, sc)
    return [
        ("sar_gpool_prep_f32", lambda: lib.sar_gpool_prep_f32(p, C * T, p, p, None)),
        ("sar_gpool_score_f32", lambda: lib.sar_gpool_score_f32(p, sn_x, sc_x, p, N, C, T, V, p, None)),
        ("sar_gpool_select_f32", lambda: lib.sar_gpool_select_f32(p, N, C, T, V, keep, p, p, p, p, None)),
        ("sar_gpool_gather_f32", lambda: lib.sar_gpool_gather_f32(p, sn_x, sc_x, p, p, N, C, T, V, keep, p, sn_o, sc_o, None)),
        ("sar_gpool_adj_f32", lambda: lib.sar_gpool_adj_f32(p, p, N, K, V, keep, p, None)),
        ("sar_gpool_adj_bwd_f32", lambda: lib.sar_gpool_adj_bwd_f32(p, p, p, p, N, K, V, keep, p, None)),
        ("sar_gpool_ds_f32", lambda: lib.sar_gpool_ds_f32(p, sn_x, sc_x, p, sn_o, sc_o, p, N, C, T, V, keep, p, None)),
        ("sar_gpool_dy_f32", lambda: lib.sar_gpool_dy_f32(p, p, p, N, C, T, V, keep, p, None)),
        ("sar_gpool_dx_f32", lambda: lib.sar_gpool_dx_f32(p, sn_x, sc_x, p, sn_o, sc_o, p, p, p, p, N, C, T, V, keep, p, sn_x, sc_x, p, None)),
        ("sar_gpool_dp_f32", lambda: lib.sar_gpool_dp_f32(p, p, p, N, C * T, p, p, None)),
    ]


def test_null_operands_are_argument_errors(lib):
    for name, call in _calls(lib, None, 2, 4, 3, 5, 2, 2):
        _rejected(lib, call(), ARG, name)


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for name, call in _calls(lib, p, 2, 4, 3, 65, 2, 2):                 # V = 65
        if name not in NO_SHAPE:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 9, 2):                  # K = 9
        if name in ADJ:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 2, 0):                  # keep = 0 (score takes no keep)
        if name not in NO_SHAPE + ("sar_gpool_score_f32",):
            _rejected(lib, call(), EITHER, name)
    for name, call in _calls(lib, p, 2, 4, 3, 5, 2, 6):                  # keep > V
        if name not in NO_SHAPE + ("sar_gpool_score_f32",):
            _rejected(lib, call(), EITHER, name)
    for name, call in _calls(lib, p, 65536, 1, 1, 5, 2, 2):              # N = 65536 (prep takes no N)
        if name != "sar_gpool_prep_f32":
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2048, 1024, 64, 25, 2, 12):         # 2^31 elements and more
        if name not in NO_SHAPE + ADJ:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 0, 3, 5, 2, 2):                  # C = 0
        if name not in ADJ:
            _rejected(lib, call(), ARG, name)
    for sn, sc in ((4 * 3 * 5, 3 * 5 - 1), (3 * 5 - 1, 2 * 3 * 5), (3 * 5, 2 * 3 * 5 - 1), (4 * 3 * 5 - 1, 3 * 5), (0, 15), (60, -15)):
        for name, call in _calls(lib, p, 2, 4, 3, 5, 2, 5, sn, sc):      # runs that overlap or run backwards (keep = V: one run length)
            if name in WALKS:
                _rejected(lib, call(), ARG, name)
    assert lib.sar_gpool_groups(64, 300) == 16 and lib.sar_gpool_groups(256, 75) == 19 and lib.sar_gpool_groups(3, 5000) == 3
    assert lib.sar_gpool_groups(0, 5) == _lib.SAR_E_ARG


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)

    def f(*shape):
        return torch.zeros(shape, dtype=torch.float32)
    N, C, T, V, K = 2, 4, 3, 5, 2
    x, A, p = f(N, C, T, V), f(N, K, V, V), f(C * T, 1)
    with pytest.raises(ValueError, match="CUDA"):                        # host tensors
        ops.gpool_forward(x, A, p, 0.5)
    with pytest.raises(ValueError, match="V <= 64"):
        ops.gpool_forward(f(N, C, T, 65), f(N, K, 65, 65), p, 0.5)
    with pytest.raises(ValueError, match="K <= 8"):
        ops.gpool_forward(x, f(N, 9, V, V), p, 0.5)
    with pytest.raises(ValueError, match="N <= 65535"):
        ops.gpool_forward(f(65536, 1, 1, V), f(1, K, V, V), f(1, 1), 0.5)
    with pytest.raises(ValueError, match="keep"):
        ops.gpool_forward(x, A, p, 0.1)
    with pytest.raises(ValueError, match="keeprate"):
        ops.gpool_forward(x, A, p, 0.0)
    with pytest.raises(ValueError, match="expand"):                      # a 3-D adjacency
        ops.gpool_forward(x, f(K, V, V), p, 0.5)
    with pytest.raises(ValueError, match="float32"):
        ops.gpool_forward(x.double(), A, p, 0.5)
    with pytest.raises(ValueError, match="inner strides"):               # a vertex stride
        ops.gpool_forward(f(N, C, T, 2 * V)[..., ::2], A, p, 0.5)
    with pytest.raises(ValueError, match="inner strides"):               # a frame stride
        ops.gpool_forward(f(N, C, 2 * T, V)[:, :, ::2], A, p, 0.5)
    with pytest.raises(ValueError, match="inner strides"):               # frame-major: neither NCHW nor CN
        ops.gpool_forward(f(T, N, C, V).permute(1, 2, 0, 3), A, p, 0.5)
    saved = (torch.zeros((N, 2), dtype=torch.int32), torch.zeros((N, V), dtype=torch.int32), f(N, V), f(N, 2), f(C * T), f(2))
    with pytest.raises(ValueError, match="CUDA"):
        ops.gpool_backward(x, A, saved, f(N, C, T, 2), f(N, K, 2, 2))
    with pytest.raises(ValueError, match="shape"):                       # dout of another keep
        ops.gpool_backward(x, A, saved, f(N, C, T, 3), None)
    assert ops.gpool_keep(0.5, 25) == 12 and ops.gpool_keep(0.7, 25) == 17 and ops.gpool_keep(0.28, 25) == 7
