"""CPU: the ABI of csrc/adjattn.hip (include/sar_hip.h, AdaptiveAdjacency).  Every sar_adjattn_* prototype of the header has a row of
matching arity and types in sar_amd/_lib.py; the entry points check pointers, sizes and leading dimensions before anything is launched,
so they answer on a machine without a GPU (SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()); the wrappers
of sar_amd/ops.py and the modules of models/agcn.py reject what the kernels are not built for before they touch the library."""
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
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(sar_adjattn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_every_prototype_has_a_binding_row_of_matching_arity_and_types():
    protos = _prototypes()
    assert set(protos) == {"sar_adjattn_sim_slabs", "sar_adjattn_sim_f32", "sar_adjattn_softmax_f32", "sar_adjattn_softmax_bwd_f32",
                           "sar_adjattn_dembed_f32"}
    assert set(protos) == {k for k in _lib.SIGNATURES if k.startswith("sar_adjattn_")}
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
EMBED = ("sar_adjattn_sim_f32", "sar_adjattn_dembed_f32")          # take Ce, T and the [K Ce][ld] matrices


def _calls(lib, p, N, K, Ce, T, V, ld=None, nslab=1):
    """the four kernels with the same sizes; p = the base of what stands in for the pointers (distinct operands 64 bytes apart);
    ld defaults to N T V"""
    ld = N * T * V if ld is None else ld
    q = [None] * 6 if p is None else [p + 64 * i for i in range(6)]
    return [
        ("sar_adjattn_sim_f32", lambda: lib.sar_adjattn_sim_f32(q[0], q[1], ld, N, K, Ce, T, V, q[2], q[3], nslab, None)),
        ("sar_adjattn_softmax_f32", lambda: lib.sar_adjattn_softmax_f32(q[0], q[1], N, K, V, q[2], q[3], None)),
        ("sar_adjattn_softmax_bwd_f32", lambda: lib.sar_adjattn_softmax_bwd_f32(q[0], q[1], N, K, V, q[2], q[3], None)),
        ("sar_adjattn_dembed_f32", lambda: lib.sar_adjattn_dembed_f32(q[0], q[1], q[2], ld, N, K, Ce, T, V, q[3], q[4], ld, None)),
    ]


def test_null_operands_are_argument_errors(lib):
    for name, call in _calls(lib, None, 2, 3, 2, 4, 5):
        _rejected(lib, call(), ARG, name)


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 128)()
    p = ctypes.addressof(buf)
    for name, call in _calls(lib, p, 2, 3, 2, 4, 33):                    # V = 33
        _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 3, 2, 4, 0):                     # V = 0
        _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 5, 2, 4, 5):                     # K = 5
        _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 0, 2, 4, 5):                     # K = 0
        _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 1, 513, 4, 5, nslab=2):          # K Ce = 513
        if name in EMBED:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 3, 171, 4, 5, nslab=1):          # K Ce = 513 again
        if name in EMBED:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 2, 3, 0, 4, 5):                     # Ce = 0
        if name in EMBED:
            _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 3, 2, 0, 5):                     # T = 0
        if name in EMBED:
            _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 3, 2, 4, 5, ld=39):              # ld < N T V = 40
        if name in EMBED:
            _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 2, 3, 2, 4, 5, ld=1 << 31):         # ld = 2^31
        if name in EMBED:
            _rejected(lib, call(), ARG, name)
    for name, call in _calls(lib, p, 1 << 7, 3, 2, 1 << 10, 32):         # N T V = 2^22
        if name in EMBED:
            _rejected(lib, call(), UNSUP, name)
    for name, call in _calls(lib, p, 21846, 3, 1, 1, 5):                 # N K = 65538
        _rejected(lib, call(), UNSUP, name)
    _rejected(lib, lib.sar_adjattn_sim_f32(p, p + 64, 40, 2, 3, 2, 4, 5, p + 128, None, 2, None), ARG, "sar_adjattn_sim_f32")       # not the slab count
    _rejected(lib, lib.sar_adjattn_sim_f32(p, p + 64, 950, 1, 1, 27, 38, 25, p + 128, None, 2, None), ARG, "sar_adjattn_sim_f32")   # two slabs, no buffer
    # an output that is an input
    a, b, c, d, e = (p + 64 * i for i in range(5))
    for rc in (lib.sar_adjattn_sim_f32(a, b, 40, 2, 3, 2, 4, 5, a, None, 1, None), lib.sar_adjattn_sim_f32(a, b, 40, 2, 3, 2, 4, 5, b, None, 1, None)):
        _rejected(lib, rc, ARG, "sar_adjattn_sim_f32")
    for rc in (lib.sar_adjattn_softmax_f32(a, b, 2, 3, 5, a, d, None), lib.sar_adjattn_softmax_f32(a, b, 2, 3, 5, c, a, None),
               lib.sar_adjattn_softmax_f32(a, b, 2, 3, 5, c, b, None), lib.sar_adjattn_softmax_f32(a, b, 2, 3, 5, c, c, None)):
        _rejected(lib, rc, ARG, "sar_adjattn_softmax_f32")
    for rc in (lib.sar_adjattn_softmax_bwd_f32(a, b, 2, 3, 5, a, None, None), lib.sar_adjattn_softmax_bwd_f32(a, b, 2, 3, 5, b, None, None),
               lib.sar_adjattn_softmax_bwd_f32(a, b, 2, 3, 5, c, b, None), lib.sar_adjattn_softmax_bwd_f32(a, b, 2, 3, 5, c, c, None)):
        _rejected(lib, rc, ARG, "sar_adjattn_softmax_bwd_f32")
    for dt, dp in ((a, e), (b, e), (c, e), (d, a), (d, b), (d, c), (d, d)):
        _rejected(lib, lib.sar_adjattn_dembed_f32(a, b, c, 40, 2, 3, 2, 4, 5, dt, dp, 40, None), ARG, "sar_adjattn_dembed_f32")


def test_slab_count_is_a_function_of_the_embedding_shape_alone(lib):
    """about 512 steps of two frames of one channel to a slab, at most 8; N and K are not even arguments"""
    slabs = lib.sar_adjattn_sim_slabs
    assert slabs(16, 300, 25) == 5 and slabs(64, 75, 25) == 5             # the workload: 2 400 and 2 432 steps
    assert slabs(1, 1, 25) == 1 and slabs(4, 40, 25) == 1 and slabs(16, 64, 7) == 1       # 512 steps: still one
    assert slabs(27, 38, 25) == 2                                         # 513 steps: the first size with two
    assert slabs(170, 300, 25) == 8 and slabs(512, 5000, 25) == 8
    assert slabs(0, 3, 25) == _lib.SAR_E_ARG and slabs(2, 3, 33) == _lib.SAR_E_UNSUP and slabs(513, 3, 25) == _lib.SAR_E_UNSUP
    assert b"sar_adjattn_sim_slabs" in lib.sar_last_error_string()


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def test_wrappers_reject_before_calling_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    N, C, T, V, K, Ce = 2, 4, 3, 5, 3, 2
    X, A, tk, pk, pb = _f(C, N * T * V), _f(K, V, V), _f(1, 1, C, K * Ce), _f(1, 1, C, K * Ce), _f(K * Ce)
    fwd = ops.adjattn_forward
    with pytest.raises(ValueError, match="CUDA"):                        # host tensors
        fwd(X, N, T, V, A, tk, pk, pb)
    with pytest.raises(ValueError, match="float32"):
        fwd(X.double(), N, T, V, A, tk, pk, pb)
    with pytest.raises(ValueError, match="CN matrix"):                   # another column count
        fwd(_f(C, N * T * V + 1), N, T, V, A, tk, pk, pb)
    with pytest.raises(ValueError, match="CN matrix"):                   # a column stride
        fwd(_f(C, 2 * N * T * V)[:, ::2], N, T, V, A, tk, pk, pb)
    with pytest.raises(ValueError, match="CN matrix"):
        fwd(_f(N, C, T, V), N, T, V, A, tk, pk, pb)
    with pytest.raises(ValueError, match=r"\(K, V, V\)"):
        fwd(X, N, T, V, _f(K, V, V + 1), tk, pk, pb)
    with pytest.raises(ValueError, match=r"\(K, V, V\)"):
        fwd(X, N, T, V, _f(N, K, V, V), tk, pk, pb)
    with pytest.raises(ValueError, match="V <= 32"):
        fwd(_f(C, N * T * 33), N, T, 33, _f(K, 33, 33), tk, pk, pb)
    with pytest.raises(ValueError, match="K <= 4"):
        fwd(X, N, T, V, _f(5, V, V), _f(1, 1, C, 10), _f(1, 1, C, 10), _f(10))
    with pytest.raises(ValueError, match="K Ce <= 512"):
        fwd(X, N, T, V, A, _f(1, 1, C, 513), _f(1, 1, C, 513), _f(513))
    with pytest.raises(ValueError, match="multiple of K"):
        fwd(X, N, T, V, A, _f(1, 1, C, 7), _f(1, 1, C, 7), _f(7))
    with pytest.raises(ValueError, match="theta_kernel"):                # a kernel for other channels
        fwd(X, N, T, V, A, _f(1, 1, C + 1, K * Ce), pk, pb)
    with pytest.raises(ValueError, match="phi_kernel"):                  # the two embeddings differ in width
        fwd(X, N, T, V, A, tk, _f(1, 1, C, K * Ce + K), pb)
    with pytest.raises(ValueError, match="phi_bias"):
        fwd(X, N, T, V, A, tk, pk, _f(K * Ce + 1))
    with pytest.raises(ValueError, match="2\\^22"):
        fwd(_f(1, 1 << 22), 1 << 7, 1 << 10, 32, _f(1, 32, 32), _f(1, 1, 1, 1), _f(1, 1, 1, 1), _f(1))
    with pytest.raises(ValueError, match="65535"):
        fwd(_f(1, 21846), 21846, 1, 1, _f(3, 1, 1), _f(1, 1, 1, 3), _f(1, 1, 1, 3), _f(3))
    saved = (_f(2 * K * Ce, N * T * V), _f(N, K, V, V))
    bwd = ops.adjattn_backward
    with pytest.raises(ValueError, match="CUDA"):
        bwd(X, N, T, V, saved, tk, pk, _f(N, K, V, V))
    with pytest.raises(ValueError, match="dA_eff"):                      # dA_eff of another shape
        bwd(X, N, T, V, saved, tk, pk, _f(N, K, V, V + 1))
    with pytest.raises(ValueError, match="saved"):
        bwd(X, N, T, V, (_f(K * Ce, N * T * V), saved[1]), tk, pk, _f(N, K, V, V))


def test_modules_reject_without_building_or_launching(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    from models.agcn import AdaptiveAdjacency, AdaptiveGraphConv
    for bad in ((171, 3), (0, 3), (2, 5), (2, 0), (513, 1)):
        with pytest.raises(ValueError, match="K Ce <= 512"):
            AdaptiveAdjacency(*bad)
    with pytest.raises(ValueError, match="K Ce <= 512"):
        AdaptiveGraphConv(8, kernel_size=5)
    m, g = AdaptiveAdjacency(2), AdaptiveGraphConv(8)
    assert (m.embed_channels, m.kernel_size) == (2, 3) and (g.adjacency.embed_channels, g.filters, g.kernel_size) == (2, 8, 3)
    assert AdaptiveGraphConv(3).adjacency.embed_channels == 1 and AdaptiveGraphConv(8, 2, 5).adjacency.embed_channels == 5
    for layer in (m, g):
        assert [n for n, _ in layer.named_parameters()] == []
        for x, A in ((_f(2, 4, 3, 5), _f(3, 5, 5)), (_f(2, 4, 15), _f(3, 5, 5))):          # host tensors, three dimensions
            with pytest.raises(ValueError, match="contiguous float32 CUDA"):
                layer(x, A, True)
        assert [n for n, _ in layer.named_parameters()] == [], "a rejected call built the parameters"
