"""CPU: the ABI of csrc/pgpool.hip (include/sar_hip.h, ProjectionGraphPool).  Every sar_pgpool_* prototype of the header has a row
of matching arity in sar_amd/_lib.py; the entry points check their arguments before anything is launched, so they answer on a
machine without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()); the wrappers of
sar_amd/ops.py reject what the kernels are not built for before they touch the library."""
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
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_pgpool_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_every_prototype_has_a_binding_row_of_matching_arity():
    protos = _prototypes()
    assert len(protos) == 13 and "sar_pgpool_assign_f32" in protos and "sar_pgpool_param_grad_f32" in protos
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_pgpool_")}
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
    assert rc == want, "%s returned %d, expected %d" % (name, rc, want)
    assert name.encode() in lib.sar_last_error_string()


def _calls(lib, p, B, P, C, J, ld):
    """every entry point with the same sizes; p = what stands in for each pointer"""
    return [
        ("sar_pgpool_prep_f32", lambda: lib.sar_pgpool_prep_f32(p, p, C, J, p, None)),
        ("sar_pgpool_assign_f32", lambda: lib.sar_pgpool_assign_f32(p, ld, B, P, C, J, p, p, p, ld, p, None)),
        ("sar_pgpool_moment_f32", lambda: lib.sar_pgpool_moment_f32(p, ld, p, ld, B, P, C, J, 0, p, None)),
        ("sar_pgpool_rowsum_f32", lambda: lib.sar_pgpool_rowsum_f32(p, ld, B, P, J, p, None)),
        ("sar_pgpool_normalize_f32", lambda: lib.sar_pgpool_normalize_f32(p, p, p, p, B, C, J, p, p, None)),
        ("sar_pgpool_gram_f32", lambda: lib.sar_pgpool_gram_f32(p, B, C, J, p, None)),
        ("sar_pgpool_gram_bwd_f32", lambda: lib.sar_pgpool_gram_bwd_f32(p, p, p, B, C, J, p, None)),
        ("sar_pgpool_normalize_bwd_f32", lambda: lib.sar_pgpool_normalize_bwd_f32(p, p, p, p, p, p, p, B, C, J, p, p, None)),
        ("sar_pgpool_dq_f32", lambda: lib.sar_pgpool_dq_f32(p, ld, p, p, B, P, C, J, p, ld, None)),
        ("sar_pgpool_softmax_bwd_f32", lambda: lib.sar_pgpool_softmax_bwd_f32(p, ld, p, B, P, J, p, ld, None)),
        ("sar_pgpool_dx_f32", lambda: lib.sar_pgpool_dx_f32(p, ld, p, p, ld, p, ld, p, B, P, C, J, p, ld, None)),
        ("sar_pgpool_param_grad_f32", lambda: lib.sar_pgpool_param_grad_f32(p, p, p, p, p, p, p, p, B, C, J, p, p, None)),
    ]


def test_null_operands_are_argument_errors(lib):
    for name, call in _calls(lib, None, 2, 8, 4, 4, 16):
        _rejected(lib, call(), _lib.SAR_E_ARG, name)


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for name, call in _calls(lib, p, 2, 8, 513, 4, 16):              # C > 512 (rowsum and softmax_bwd take no C)
        if name not in ("sar_pgpool_rowsum_f32", "sar_pgpool_softmax_bwd_f32"):
            _rejected(lib, call(), _lib.SAR_E_UNSUP, name)
    for name, call in _calls(lib, p, 2, 8, 4, 513, 16):              # J > 512
        _rejected(lib, call(), _lib.SAR_E_UNSUP, name)
    for name, call in _calls(lib, p, 65536, 8, 4, 4, 1 << 20):       # B > 65535 (prep takes no B)
        if name != "sar_pgpool_prep_f32":
            _rejected(lib, call(), _lib.SAR_E_UNSUP, name)
    for name, call in _calls(lib, p, 2, 8, 4, 0, 16):                # J = 0
        _rejected(lib, call(), _lib.SAR_E_ARG, name)
    for name, call in _calls(lib, p, 2, 8, 4, 4, 15):                # ld < B P, where there is an ld
        if name in ("sar_pgpool_assign_f32", "sar_pgpool_moment_f32", "sar_pgpool_rowsum_f32", "sar_pgpool_dq_f32",
                    "sar_pgpool_softmax_bwd_f32", "sar_pgpool_dx_f32"):
            _rejected(lib, call(), _lib.SAR_E_ARG, name)
    assert lib.sar_pgpool_clamp_words(512) == 16 and lib.sar_pgpool_clamp_words(24) == 2 and lib.sar_pgpool_clamp_words(65) == 4
    assert lib.sar_pgpool_clamp_words(0) == 0


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    def f(*shape):
        return torch.zeros(shape, dtype=torch.float32)
    B, P = 2, 3
    with pytest.raises(ValueError, match="C <= 512"):                # C > 512
        ops.pgpool_forward(f(513, B * P), B, P, f(513 * 4), f(513 * 4))
    with pytest.raises(ValueError, match="J <= 512"):                # J > 512
        ops.pgpool_forward(f(4, B * P), B, P, f(4 * 513), f(4 * 513))
    with pytest.raises(ValueError, match="unit column stride"):      # x with a column stride
        ops.pgpool_forward(f(4, 2 * B * P)[:, ::2], B, P, f(16), f(16))
    with pytest.raises(ValueError, match="contiguous"):              # strided parameters
        ops.pgpool_forward(f(4, B * P), B, P, f(32)[::2], f(16))
    with pytest.raises(ValueError, match="CUDA"):                    # a host tensor
        ops.pgpool_forward(f(4, B * P), B, P, f(16), f(16))
    saved = (f(4, B * P), torch.zeros((B * P, 2), dtype=torch.int32), f(B, 4, 4), f(B, 4), f(B, 4), f(4, 4, 4))
    with pytest.raises(ValueError, match="unit column stride"):      # dx with a column stride
        ops.pgpool_backward(f(4, B * P), B, P, f(16), f(B, 4, 4), saved, f(B, 4, 4), f(B, 4, 4), f(4, 2 * B * P)[:, ::2], f(16), f(16))
    with pytest.raises(ValueError, match="contiguous"):              # dz strided
        ops.pgpool_backward(f(4, B * P), B, P, f(16), f(B, 4, 4), saved, f(B, 4, 8)[:, :, ::2], f(B, 4, 4), f(4, B * P), f(16), f(16))
