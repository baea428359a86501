"""CPU: the ABI of the skeleton gradient of the VirtualRadar signal stage (include/sar_hip.h: sar_vr_signal_bwd_x_f32).  The symbol
is declared, exported and bound with a row of matching arity and types in sar_amd/_lib.py; every argument check runs before the
launch, so the rejections answer on a machine without a GPU (SAR_E_ARG with the entry point named in sar_last_error_string()); a
small integer stands in for a device pointer, a rejected call dereferences nothing."""
import ctypes
import os
import re

import pytest

from sar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sar_vr_signal_bwd_x_f32"
P = 4096        # stands in for an aligned device pointer


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_the_entry_point_is_declared_bound_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sar_hip.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert len(protos) == 1
    params = [a.strip() for a in protos[0].split(",") if a.strip()]
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(argtypes) == len(params) == 14, (len(argtypes), len(params))
    for a, ty in zip(params, argtypes):
        want = ctypes.c_void_p if ("*" in a or "sar_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
        assert ty is want, (a, ty)
    assert hasattr(lib, NAME)
    # the same operands in the same order as its sibling for (loc, wavelength), with dx in place of the partial sums
    sib = re.findall(r"\bint\s+sar_vr_signal_bwd_f32\s*\(([^)]*)\)\s*;", hdr)[0]
    assert [re.sub(r"\w+$", "", a.strip()) for a in sib.split(",")] == [re.sub(r"\w+$", "", a) for a in params]


def _call(lib, x=P, B=2, T=9, V=25, M=2, e_src=P, e_dst=P, E=24, loc=P, wavelength=P, dz_re=P, dz_im=P, dx=P):
    return getattr(lib, NAME)(x, B, T, V, M, e_src, e_dst, E, loc, wavelength, dz_re, dz_im, dx, None)


def _rejected(lib, **kw):
    rc = _call(lib, **kw)
    assert rc == _lib.SAR_E_ARG, "%s(%s) returned %d" % (NAME, kw, rc)
    assert NAME.encode() in lib.sar_last_error_string(), lib.sar_last_error_string()


def test_null_operands_are_argument_errors(lib):
    for operand in ("x", "e_src", "e_dst", "loc", "wavelength", "dz_re", "dz_im", "dx"):
        _rejected(lib, **{operand: None})


def test_sizes_are_checked_before_any_launch(lib):
    for size in ("B", "T", "V", "M", "E"):
        _rejected(lib, **{size: 0})
        _rejected(lib, **{size: -1})
    _rejected(lib, M=5)                                          # at most four bodies
    _rejected(lib, V=42, M=1)                                    # two one-body slabs of 3 * 64 * 43 floats: 66 048 bytes
    _rejected(lib, V=100, M=4)                                   # V*M = 400
    _rejected(lib, V=1 << 30, M=4)                               # (the slab size does not wrap)
    _rejected(lib, V=25, M=2, E=1 << 14)                         # the edge lists share the 64 KB
    _rejected(lib, B=65536)
    _rejected(lib, B=1, T=715827883, V=1, M=1)                   # 3 T = 2^31 + 1 elements
    _rejected(lib, B=32768, T=1 << 10, V=16, M=4)                # 3 * 2^31
    _rejected(lib, B=65535, T=(1 << 31) - 1, V=41, M=4)          # (the product does not wrap)
