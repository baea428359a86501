"""CPU: the ABI of the backward apply pass of data_bn (include/sar_hip.h: sar_data_bn_bwd_apply_f32 / _cn8).  Both symbols are
exported with a row of matching arity in sar_amd/_lib.py; every argument check runs before the launch, so the rejections answer on a
machine without a GPU (SAR_E_ARG with the entry point named in sar_last_error_string()); a small integer stands in for a device
pointer, a rejected call dereferences nothing.  (The bone table is device memory: its entries are checked where the table is built,
sar_amd.stgcn.STGCN.)"""
import ctypes
import os
import re

import pytest

from sar_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sar_data_bn_bwd_apply_f32", "sar_data_bn_bwd_apply_cn8")
P = 4096        # stands in for an aligned device pointer


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_both_entry_points_are_declared_bound_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sar_hip.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_data_bn_bwd_apply_[a-z0-9]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(NAMES)
    for name, args in protos.items():
        params = [a.strip() for a in args.split(",") if a.strip()]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(params) == 15, (name, len(argtypes), len(params))
        for a, ty in zip(params, argtypes):
            want = ctypes.c_void_p if ("*" in a or "sar_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
            assert ty is want, (name, a, ty)
        assert hasattr(lib, name)


def test_the_frame_chunk_is_exported(lib):
    assert lib.sar_data_bn_dx_frames() == ops.DATA_BN_DX_FRAMES >= 1


def _call(lib, name, x=P, N=2, C=3, T=5, V=25, M=2, dy=P, ld=None, k1=P, k2=P, k3=P, dx=P, motion=1, parent=P):
    ld = N * M * T * V if ld is None else ld
    return getattr(lib, name)(x, N, C, T, V, M, parent, motion, dy, ld, k1, k2, k3, dx, None)


def _rejected(lib, name, **kw):
    rc = _call(lib, name, **kw)
    assert rc == _lib.SAR_E_ARG, "%s(%s) returned %d" % (name, kw, rc)
    assert name.encode() in lib.sar_last_error_string(), lib.sar_last_error_string()


@pytest.mark.parametrize("name", NAMES)
def test_null_operands_are_argument_errors(lib, name):
    for operand in ("x", "dy", "k1", "k2", "k3", "dx"):
        _rejected(lib, name, **{operand: None})


@pytest.mark.parametrize("name", NAMES)
def test_sizes_and_the_leading_dimension_are_checked_before_any_launch(lib, name):
    for size in ("N", "C", "T", "V", "M"):
        _rejected(lib, name, **{size: 0})
        _rejected(lib, name, **{size: -1})
    _rejected(lib, name, ld=2 * 2 * 5 * 25 - 1)                  # ld_dy < N*M*T*V
    _rejected(lib, name, ld=0)
    _rejected(lib, name, V=129, M=2)                             # V*M = 258 > 256 threads per workgroup
    _rejected(lib, name, V=65536, M=65536)                       # (the product does not wrap)
    _rejected(lib, name, N=1, V=1, M=256, T=1 << 24)             # a slab of 2^32 elements
    _rejected(lib, name, N=1 << 20, C=8, T=1 << 12, V=1, M=1)    # 2^31 workgroups


def test_the_cn8_plane_holds_at_most_eight_channels(lib):
    _rejected(lib, "sar_data_bn_bwd_apply_cn8", C=9)
