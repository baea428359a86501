"""Records what crosses the C ABI (include/sar_hip.h) while the tensor-level wrappers of sar_amd run on CPU tensors: a proxy that
stands in for the loaded library, passes the host-only query entry points through to it and records every other call WITHOUT
launching anything -- on a machine with a GPU as well as on one without.  A helper of tests/test_conv_launch_abi.py,
tests/test_layer_launch_abi.py and their generators under tests/golden/, not a test.

    with AbiTrace() as tr:
        ops.conv_gemm(...)
    tr.calls        # [{"fn": "sar_conv_gemm_f32", "args": [{"desc": "ConvDesc", "mode": 1, ..., "src": "p0", ...}, None]},
                    #  {"ret": "ops.conv_gemm", "value": None}]

A recorded call is the entry point's name, its scalar arguments, every field of a `byref` descriptor by name, and every pointer --
argument or descriptor field -- as p<k> in order of first appearance within the trace (None stays None), so a trace depends on no
address.  Every tensor whose address is taken stays alive until the trace ends: no two of them can share an address.  The item
tables of the batched launches are host memory in these runs and are decoded from their address.  The convolution wrappers also
leave what they return: None, or (the shape of the partials, nparts)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sar_amd import _lib as L  # noqa: E402
from sar_amd import ops, ops8  # noqa: E402

# entry points that only compute a number on the host: passed through, not recorded
_QUERY_SUFFIXES = ("_nparts", "_blocks", "_bytes", "_floats", "_frames", "_groups", "_words", "_slabs")
_QUERY_NAMES = ("sar_struct_size", "sar_version", "sar_last_error_string")
# the item table of a batched launch: (its argument, the argument that counts its items, the item's record, the pointer fields)
_TABLES = {
    "sar_slab_reduce_batch_f32": (0, 1, ops.SlabBatch.ITEM, ("slab", "out")),
    "sar_pack_weights_bf16_batch": (1, 2, ops.PackedWeights.ITEM, ()),
    "sar_pack_weights_split_batch": (1, 2, ops.PackedWeights.ITEM, ()),
    "sar_permute3_batch_f32": (2, 3, ops.PermuteBatch.ITEM, ()),
}
# a host array of int32 handed over as a void pointer: (its argument, the argument that counts its elements)
_HOST_INTS = {"sar_graph_gather_sum_f32": (4, 6), "sar_graph_gather_expand_f32": (4, 5)}
# the wrappers whose return value is recorded
WRAPPERS = ((ops, "conv_gemm"), (ops, "conv_wgrad"), (ops, "conv_gemm_nparts"), (ops, "conv2d_gemm"), (ops, "conv2d_wgrad"),
            (ops8, "conv_gemm"), (ops8, "conv_wgrad"))


def is_query(name):
    return name.endswith(_QUERY_SUFFIXES) or name in _QUERY_NAMES


def _scalar(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, bytes):
        return v.decode()
    if hasattr(v, "value"):      # a ctypes scalar
        return _scalar(v.value)
    return float(v) if isinstance(v, (np.floating, torch.Tensor)) else int(v)


class AbiTrace:
    """the recording proxy, as a context manager: installs itself as sar_amd._lib._lib, stubs the three stream_ptr names (no
    stream: None), lets every tensor answer is_cuda = True, and restores all of it on exit"""

    def __init__(self):
        self.calls, self._names, self._alive, self._undo = [], {}, [], []

    # ---- naming
    def pointer(self, p):
        if isinstance(p, C.c_void_p):
            p = p.value
        if p is None:
            return None
        return self._names.setdefault(int(p), "p%d" % len(self._names))

    def _struct(self, s):
        rec = {"desc": type(s).__name__}
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ is C.c_void_p:
                rec[name] = self.pointer(v)
            elif isinstance(v, C.Array):
                rec[name] = [_scalar(e) for e in v]
            else:
                rec[name] = _scalar(v)
        return rec

    def _table(self, addr, count, item, pointers):
        dt = np.dtype(item, align=True)
        raw = (C.c_char * (count * dt.itemsize)).from_address(addr)
        tab = np.frombuffer(raw, dtype=dt, count=count)
        return [{n: (self.pointer(int(row[n])) if n in pointers else int(row[n])) for n in dt.names if n != "reserved"} for row in tab]

    def _arg(self, name, k, a, typ, args):
        if name in _TABLES and k == _TABLES[name][0]:
            _, cnt, item, pointers = _TABLES[name]
            return {"table": self._table(a, args[cnt], item, pointers)}
        if name in _HOST_INTS and k == _HOST_INTS[name][0]:
            n = args[_HOST_INTS[name][1]]
            return {"ints": list((C.c_int32 * n).from_address(a.value if isinstance(a, C.c_void_p) else a))}
        if hasattr(a, "_obj"):      # C.byref(..): a descriptor, or a cell the library writes its answer to
            return self._struct(a._obj) if isinstance(a._obj, C.Structure) else {"out": type(a._obj).__name__}
        if isinstance(a, C.Array):      # host words (a CU mask)
            return {"words": [_scalar(e) for e in a]}
        if typ is C.c_void_p or isinstance(a, C.c_void_p):
            return self.pointer(a)
        return _scalar(a)

    # ---- the library's stand-in
    def __getattr__(self, name):
        if name.startswith("_") or name not in L.SIGNATURES:
            raise AttributeError(name)
        if is_query(name):
            return getattr(self._real, name)
        types = L.SIGNATURES[name][1]

        def record(*args):
            assert len(args) == len(types), "%s takes %d arguments, got %d" % (name, len(types), len(args))
            self.calls.append({"fn": name, "args": [self._arg(name, k, a, types[k], args) for k, a in enumerate(args)]})
            return 0
        return record

    def _returns(self, owner, name):
        fn = getattr(owner, name)
        tag = "%s.%s" % (owner.__name__.rsplit(".", 1)[-1], name)

        def wrapper(*a, **k):
            r = fn(*a, **k)
            self.calls.append({"ret": tag, "value": [list(r[0].shape), int(r[1])] if isinstance(r, tuple) else _scalar(r)})
            return r
        return wrapper

    # ---- installation
    def _set(self, owner, name, value):
        had = name in vars(owner)
        self._undo.append((owner, name, had, vars(owner).get(name)))
        setattr(owner, name, value)

    def __enter__(self):
        L._lib = None
        self._real = L.load()
        self._set(L, "_lib", self)
        for mod in (L, ops, ops8):
            self._set(mod, "stream_ptr", lambda: None)
        self._set(torch.Tensor, "is_cuda", property(lambda t: True))
        data_ptr, alive = torch.Tensor.data_ptr, self._alive

        def keep(t):
            alive.append(t)
            return data_ptr(t)
        self._set(torch.Tensor, "data_ptr", keep)
        for owner, name in WRAPPERS:
            self._set(owner, name, self._returns(owner, name))
        return self

    def __exit__(self, *exc):
        for owner, name, had, value in reversed(self._undo):
            if had:
                setattr(owner, name, value)
            else:
                delattr(owner, name)
        self._undo, self._alive = [], []
        return False
