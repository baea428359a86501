"""CPU: the ABI of csrc/pgc.hip (include/sar_hip.h, ProjectionGraphConv).  Every sar_pgc_* prototype of the header has a row of
matching arity in sar_amd/_lib.py; the entry points check their arguments before anything is launched, so they answer on a machine
without a GPU (SAR_E_ARG with the entry point named in sar_last_error_string()); the wrappers of sar_amd/ops.py reject what the
kernels are not built for with a ValueError before they touch the library.  tests/test_gpu_pgc_edges.py repeats the rejected calls
between guarded buffers."""
import ctypes
import os
import re
import types

import pytest
import torch

import pgc_cases as K
from sar_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_prototype_has_a_binding_row_of_matching_arity():
    hdr = open(os.path.join(ROOT, "include", "sar_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_pgc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert len(protos) == 8 and set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_pgc_")}
    for name, args in protos.items():
        params = [a.strip() for a in args.split(",") if a.strip()]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for a, ty in zip(params, argtypes):          # pointers cross as void*, int64_t as c_int64, int as c_int
            want = ctypes.c_void_p if ("*" in a or "sar_stream_t" in a) else ctypes.c_int64 if "int64_t" in a else ctypes.c_int
            assert ty is want, (name, a, ty)


def test_rejected_arguments_answer_without_a_gpu():
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    B, P = 2, 8
    names = ("x", "dout", "out", "dx", "cen", "var", "W", "bias", "q", "fpart", "dpart", "cpart", "saved", "dsaved", "slab", "colsum",
             "pooled", "gc", "gv")
    good = dict({k: p for k in names}, B=B, P=P, nparts=1, ld_x=B * P, ld_dout=B * P + 3, ld_out=B * P, ld_dx=B * P + 1)
    for name, (call, ptrs, lds, has_B, has_P, has_nparts) in K.entry_points(lib).items():
        bad = [{k: None} for k in ptrs] + [{k: B * P - 1} for k in lds]
        bad += [{"B": 0}, {"B": -1}, {"B": 65536, **{k: 65536 * P for k in lds}}] if has_B else []
        bad += [{"P": 0}, {"P": -3}] if has_P else []
        bad += [{"nparts": 0}, {"nparts": -1}] if has_nparts else []
        for change in bad:
            rc = call(types.SimpleNamespace(**dict(good, **change)))
            assert rc == _lib.SAR_E_ARG, "%s with %s returned %d" % (name, change, rc)
            assert name[:-4].encode() in lib.sar_last_error_string(), (name, change)
    assert [lib.sar_pgc_nparts(v) for v in (-1, 0, 1, 128, 129, 512, 513, 1024, 1025)] == [0, 0, 1, 1, 1, 1, 2, 2, 3]


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)

    def f(*shape):
        return torch.zeros(shape, dtype=torch.float32)
    B, P = 2, 3
    prm = (f(1, 64, 1, 32), f(1, 64, 1, 32), f(1, 64, 64), f(64))
    with pytest.raises(ValueError, match="CUDA"):                    # a host tensor
        ops.pgc_forward(f(64, B * P), B, P, *prm, f(64, B * P))
    with pytest.raises(ValueError, match="float32"):
        ops.pgc_forward(f(64, B * P).double(), B, P, *prm, f(64, B * P))
    with pytest.raises(ValueError, match="B >= 1 and P >= 1"):
        ops.pgc_forward(f(64, B * P), 0, P, *prm, f(64, B * P))
    with pytest.raises(ValueError, match="CUDA"):
        ops.pgc_backward(f(64, B * P), f(64, B * P), f(32, B * P), f(B, 11360), B, P, *prm[:3], f(64, B * P), f(64, 32), f(64, 32), f(4160))
