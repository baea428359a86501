"""GPU: every entry point of csrc/adjattn.hip on operands that are views into larger allocations (tests/util.py: Launch, drive).  The
stacked embeddings [2 K Ce][N T V] (theta's rows, then phi's) and their gradient are CN matrices with guard rows in front and behind and
`pad` columns of margin at the right of every row; A, the logits, P, A_eff, dA_eff, dS, dA and the slabs are flat ranges between guard
elements.  Inputs are surrounded by NaN -- whatever reads the margin and lets it reach a result shows --, outputs by a sentinel that has
to survive.  Asserted per launch: the guards are untouched, the inputs are unmodified, every output is finite, the padded run is bitwise
the unpadded one, and both are bitwise what sar_amd.ops.adjattn_forward / adjattn_backward give on plain tensors."""
import pytest
import torch

import adjattn_cases as K
from util import Launch, drive, to_cn

pytestmark = pytest.mark.gpu


class Kept(Launch):
    KEEP_INPUTS = True


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def layer(dev, case):
    """the four entry points of the layer, every buffer a guarded view"""
    from sar_amd import _lib as L
    from sar_amd import ops
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, T, V, Kk, Ce, _ = case
    x, A, tk, pk, pb, dA_eff = (t.to(torch.float32).to(dev).contiguous() for t in K.reference(case)[0])
    X, tk, pk = to_cn(x), tk.reshape(1, 1, C, -1), pk.reshape(1, 1, C, -1)
    kf, kb = {}, {}
    A_eff0, (E0, P0) = ops.adjattn_forward(X, N, T, V, A, tk, pk, pb, keep=kf)
    dA0 = ops.adjattn_backward(X, N, T, V, (E0, P0), tk, pk, dA_eff, keep=kb)[4]
    n, kce, size = N * T * V, Kk * Ce, N * Kk * V * V

    def fn(g):
        lib, st = L.load(), stream_ptr()
        E, Ain, dd = g.inp(E0), g.flat_in(A), g.flat_in(dA_eff)
        S, P, A_eff, dS, dA = g.flat("S", size), g.flat("P", size), g.flat("A_eff", size), g.flat("dS", size), g.flat("dA", Kk * V * V)
        dE = g.out("dE", 2 * kce, n)
        nslab = lib.sar_adjattn_sim_slabs(Ce, T, V)
        slab = g.flat("slab", nslab * size) if nslab > 1 else None
        ld, ld_d = E.stride(0), dE.stride(0)
        assert ld == n + g.pad == ld_d
        check(lib.sar_adjattn_sim_f32(ptr(E), ptr(E[kce:]), ld, N, Kk, Ce, T, V, ptr(S), ptr(slab), nslab, st), "sim")
        check(lib.sar_adjattn_softmax_f32(ptr(S), ptr(Ain), N, Kk, V, ptr(P), ptr(A_eff), st), "softmax")
        check(lib.sar_adjattn_softmax_bwd_f32(ptr(P), ptr(dd), N, Kk, V, ptr(dS), ptr(dA), st), "softmax_bwd")
        check(lib.sar_adjattn_dembed_f32(ptr(dS), ptr(E), ptr(E[kce:]), ld, N, Kk, Ce, T, V, ptr(dE), ptr(dE[kce:]), ld_d, st), "dembed")
        for what, got, want in (("S", S, kf["S"]), ("P", P, P0), ("A_eff", A_eff, A_eff0), ("dS", dS, kb["dS"]), ("dA", dA, dA0),
                                ("dE", dE, kb["dE"])):
            g.ref(what, got, want.reshape(got.shape), 0)
    return fn


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("case", K.SMALL + [K.EDGES[0]], ids=K.case_id)
def test_every_kernel_between_guards(dev, case, pad):
    drive(dev, layer(dev, case), pad, launch=Kept)
