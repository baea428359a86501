"""CPU: the ABI of the block tail (include/sar_hip.h: BatchNorm + residual + ReLU forward, its backward reduction, its backward
apply, affine2; fp32 and CN8).  One entry point per pass, the mask / amax cells / tail as optional pointers: each of the 8 prototypes
has a row of matching arity in sar_amd/_lib.py and none of the per-flag variants is left.  Every argument check runs before the
launch, so the rejections answer on a machine without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in
sar_last_error_string()); small integers stand in for device pointers, a rejected call dereferences nothing."""
import ctypes
import os
import re

import pytest

from sar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("sar_bn_add_relu_fwd", "sar_bn_add_relu_bwd_reduce", "sar_bn_add_relu_bwd_apply", "sar_affine2")
ENTRY_POINTS = tuple(p + sfx for sfx in ("_f32", "_cn8") for p in PASSES)
# the variants there used to be: pass + flags + layout
VARIANTS = {"_f32": (("mask", "mask_amax"), ("mask", "tail"), ("mask", "mask_amax"), ("amax",)),
            "_cn8": (("mask",), ("mask", "tail"), ("mask",), ())}
REMOVED = tuple("%s_%s%s" % (p, flags, sfx) for sfx, per_pass in VARIANTS.items() for p, fl in zip(PASSES, per_pass) for flags in fl)


def _header():
    return open(os.path.join(ROOT, "include", "sar_hip.h")).read()


def test_every_prototype_has_a_binding_row_of_matching_arity():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_(?:bn_add_relu|affine2)_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(protos) == set(ENTRY_POINTS) and len(ENTRY_POINTS) == 8
    assert {k for k in _lib.SIGNATURES if k.startswith(("sar_bn_add_relu_", "sar_affine2_"))} == set(ENTRY_POINTS)
    for name, args in protos.items():
        params = [a.strip() for a in args.split(",") if a.strip()]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for a, ty in zip(params, argtypes):          # pointers cross as void*, int64_t as c_int64, int as c_int
            want = (ctypes.POINTER(_lib.BnTail) if "sar_bn_tail" in a else ctypes.c_void_p if ("*" in a or "sar_stream_t" in a)
                    else ctypes.c_int64 if "int64_t" in a else ctypes.c_int)
            assert ty is want, (name, a, ty)


def test_the_per_flag_variants_are_gone():
    assert len(REMOVED) == 11
    hdr = _header()
    for name in REMOVED:
        assert name not in hdr and name not in _lib.SIGNATURES, name


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


P = 4096        # stands in for an aligned device pointer


def _tail(**fields):
    t = _lib.BnTail()
    t.count = 10.0
    for f in ("ticket", "gamma", "rstd", "dgamma", "dbeta", "k1", "k2", "k3", "rgamma", "rrstd", "rdgamma", "rdbeta", "rk1", "rk2", "rk3"):
        setattr(t, f, P)
    for f, v in fields.items():
        setattr(t, f, v)
    return t


def _fwd(lib, sfx, p=P, mask=None, amax=None, res_kind=2, C=3, n=8, ld=8, u=None):
    u = p if u is None else u
    head = (u, p, p, res_kind, p, p, p, p, mask)
    return getattr(lib, "sar_bn_add_relu_fwd" + sfx)(*(head + ((amax,) if sfx == "_f32" else ()) + (C, n, ld, None)))


def _reduce(lib, sfx, p=P, y=P, mask=None, partials=P, tail=None, C=3, n=8, ld=8, u=None):
    u = p if u is None else u
    return getattr(lib, "sar_bn_add_relu_bwd_reduce" + sfx)(p, y, mask, u, p, p, p, partials, 2, C, n, ld,
                                                            ctypes.byref(tail) if tail is not None else None, None)


def _apply(lib, sfx, p=P, y=P, mask=None, dr=P, amax_du=None, amax_dr=None, C=3, n=8, ld=8, u=None):
    u = p if u is None else u
    head = (p, y, mask, u, p, p, p, p, p, p, p, p, dr, p)
    return getattr(lib, "sar_bn_add_relu_bwd_apply" + sfx)(*(head + ((amax_du, amax_dr) if sfx == "_f32" else ()) + (C, n, ld, None)))


def _affine2(lib, sfx, p=P, amax=None, C=3, n=8, ld=8, a=None):
    a = p if a is None else a
    return getattr(lib, "sar_affine2" + sfx)(*((a, p, p, p, p, p) + ((amax,) if sfx == "_f32" else ()) + (C, n, ld, None)))


def _rejected(lib, rc, want, name):
    assert rc == want, "%s returned %d, expected %d" % (name, rc, want)
    assert name.encode() in lib.sar_last_error_string()


ROW_PASSES = (("sar_bn_add_relu_fwd", _fwd), ("sar_bn_add_relu_bwd_reduce", _reduce), ("sar_bn_add_relu_bwd_apply", _apply))
ALL_PASSES = ROW_PASSES + (("sar_affine2", _affine2),)


@pytest.mark.parametrize("sfx", ["_f32", "_cn8"])
def test_null_operands_and_bad_sizes_are_argument_errors(lib, sfx):
    all_null = ({}, {"y": None, "partials": None}, {"y": None, "dr": None}, {})
    for (name, call), more in zip(ALL_PASSES, all_null):
        _rejected(lib, call(lib, sfx, p=None, **more), _lib.SAR_E_ARG, name + sfx)      # all NULL
        _rejected(lib, call(lib, sfx, n=8, ld=4), _lib.SAR_E_ARG, name + sfx)           # ld < n
        _rejected(lib, call(lib, sfx, C=0), _lib.SAR_E_ARG, name + sfx)
    _rejected(lib, _fwd(lib, sfx, res_kind=3), _lib.SAR_E_ARG, "sar_bn_add_relu_fwd" + sfx)
    _rejected(lib, _fwd(lib, sfx, res_kind=-1), _lib.SAR_E_ARG, "sar_bn_add_relu_fwd" + sfx)


@pytest.mark.parametrize("sfx", ["_f32", "_cn8"])
def test_the_backward_passes_need_y_or_a_mask(lib, sfx):
    _rejected(lib, _reduce(lib, sfx, y=None, mask=None), _lib.SAR_E_ARG, "sar_bn_add_relu_bwd_reduce" + sfx)
    _rejected(lib, _apply(lib, sfx, y=None, mask=None), _lib.SAR_E_ARG, "sar_bn_add_relu_bwd_apply" + sfx)


def test_fp32_rows_with_a_mask_are_float4_rows(lib):
    for name, call in ROW_PASSES:
        _rejected(lib, call(lib, "_f32", mask=P, n=6, ld=8), _lib.SAR_E_UNSUP, name + "_f32")        # n no multiple of 4
        _rejected(lib, call(lib, "_f32", mask=P, n=8, ld=10), _lib.SAR_E_UNSUP, name + "_f32")       # ld no multiple of 4
        _rejected(lib, call(lib, "_f32", mask=P, n=8, ld=8, u=20), _lib.SAR_E_UNSUP, name + "_f32")  # a tensor at address 20


def test_amax_dr_needs_dr(lib):
    _rejected(lib, _apply(lib, "_f32", dr=None, amax_du=P, amax_dr=P), _lib.SAR_E_ARG, "sar_bn_add_relu_bwd_apply_f32")
    _rejected(lib, _apply(lib, "_f32", dr=None, mask=P, amax_dr=P), _lib.SAR_E_ARG, "sar_bn_add_relu_bwd_apply_f32")


@pytest.mark.parametrize("sfx", ["_f32", "_cn8"])
def test_the_tail_is_checked(lib, sfx):
    name = "sar_bn_add_relu_bwd_reduce" + sfx
    _rejected(lib, _reduce(lib, sfx, tail=_lib.BnTail()), _lib.SAR_E_ARG, name)                  # all NULL: no ticket
    _rejected(lib, _reduce(lib, sfx, tail=_tail(ticket=None)), _lib.SAR_E_ARG, name)
    _rejected(lib, _reduce(lib, sfx, tail=_tail(count=0.0)), _lib.SAR_E_ARG, name)
    for f in ("rstd", "k1", "k2", "k3", "rrstd", "rk1", "rk2", "rk3"):                           # (r is given: the residual branch's too)
        _rejected(lib, _reduce(lib, sfx, tail=_tail(**{f: None})), _lib.SAR_E_ARG, name)
    _rejected(lib, _reduce(lib, sfx, tail=_tail(), partials=8), _lib.SAR_E_ARG, name)            # partials at address 8


def test_cn8_tensors_are_16_byte_aligned(lib):
    for name, call in ROW_PASSES:
        _rejected(lib, call(lib, "_cn8", u=8), _lib.SAR_E_ARG, name + "_cn8")
        _rejected(lib, call(lib, "_cn8", u=8, mask=P), _lib.SAR_E_ARG, name + "_cn8")
    _rejected(lib, _affine2(lib, "_cn8", a=8), _lib.SAR_E_ARG, "sar_affine2_cn8")
