"""Writes tests/golden/layer_launch_abi.json: what the layer wrappers at the bottom of sar_amd.ops -- pgc_*, pgpool_*, gpool_*, tattn_*,
adjattn_* -- and the shared 1x1 product (ops.conv1x1_fwd / conv1x1_wgrad / conv1x1_dgrad over ops.column_geometry) hand to the C ABI:
every entry point in issue order with its scalars, leading dimensions, pointer offsets and pointer identities (tests/abi_trace.py),
for stand-alone calls through every branch of each wrapper and for one training forward + backward of the modules built on them.
Everything runs on zero-filled CPU tensors, row-padded wherever a wrapper takes a leading dimension; nothing is launched.

The fixture was written ONCE, at commit 1c0cd2e ("Add AdaptiveAdjacency and AdaptiveGraphConv on new fp32 MFMA kernels"), the parent
of the change that gave the wrappers one operand checker (sar_amd/operands.py) and moved the 1x1 product below the models, with no
SAR_* knob set.  At that commit the four 1x1 helpers were private names of models/gcn.py; the cases reach them by their present
names.  It is never regenerated from the code under test: tests/test_layer_launch_abi.py imports cases() from here and replays them.

Modules left out because they cannot be built under the trace on a machine without a GPU: AdjGraphConv (its constructor moves the
adjacency to the GPU).  Its Function is _ConvContractFn with the dense contraction, which "module GraphConvTD dense" runs; its
wrappers are those of the direct cases.

Cases, record, digest and the fixture's format are make_golden_conv_launch_abi's."""
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_golden_conv_launch_abi as G  # noqa: E402  (puts the repository and tests/ on sys.path)

import torch  # noqa: E402

COMMIT = "1c0cd2e"
Z, rows, record, digest, first_difference = G.Z, G.rows, G.record, G.digest, G.first_difference
FULL = ("pgc padded", "pgpool bwd dz dA", "gpool cn views dout dA_out", "tattn L3 dx views", "adjattn 4-d dx dA", "conv1x1 dgrad masked out")


def cn4(C, N, T, W):
    """the (N, C, T, W) view of a row-padded CN matrix [C][N T W + 4]"""
    return rows(C, N * T * W).view(C, N, T, W).permute(1, 0, 2, 3)


def _name(*parts):
    return " ".join(p for p in parts if p)


# ------------------------------------------------------------------------------------------------ ProjectionGraphConv / Pool
def _pgc():
    from sar_amd import ops
    B, P = 2, 51
    prm = Z(64, 32), Z(64, 32), Z(64, 64)
    x, out, dout, dx = (rows(64, B * P) for _ in range(4))
    q, saved = ops.pgc_forward(x, B, P, *prm, Z(64), out)
    ops.pgc_backward(x, dout, q, saved, B, P, *prm, dx, Z(64, 32), Z(64, 32), Z(64 * 64 + 64))


def _pgpool(dz, dA):
    def run():
        from sar_amd import ops
        C, J, B, P = 5, 3, 2, 7
        x, cen = rows(C, B * P), Z(C, J)
        zn, _, saved = ops.pgpool_forward(x, B, P, cen, Z(C, J))
        ops.pgpool_backward(x, B, P, cen, zn, saved, Z(B, C, J) if dz else None, Z(B, J, J) if dA else None, rows(C, B * P), Z(C, J),
                            Z(C, J))
    return run


def pg_cases():
    yield "pgc padded", _pgc
    for dz, dA in ((True, False), (False, True), (True, True)):
        yield _name("pgpool bwd", dz and "dz", dA and "dA"), _pgpool(dz, dA)


# ------------------------------------------------------------------------------------------------ GPool
def _gpool(cn, views, with_dout, with_dA):
    def run():
        from sar_amd import ops
        N, C, T, V, K, keep = 2, 3, 4, 5, 2, 3
        new = (lambda W: cn4(C, N, T, W)) if cn else (lambda W: Z(N, C, T, W))
        x, A = new(V), Z(N, K, V, V)
        out, A_out, saved = ops.gpool_forward(x, A, Z(C, T), 0.6, out=new(keep) if views else None)
        assert tuple(out.shape) == (N, C, T, keep)
        ops.gpool_backward(x, A, saved, new(keep) if with_dout else None, Z(N, K, keep, keep) if with_dA else None,
                           dx=new(V) if views else None)
    return run


def gpool_cases():
    for cn, views, (d, a) in itertools.product((False, True), (False, True), ((True, False), (False, True), (True, True))):
        yield _name("gpool", "cn" if cn else "nchw", views and "views", d and "dout", a and "dA_out"), _gpool(cn, views, d, a)


# ------------------------------------------------------------------------------------------------ TemporalAttention
def _tattn(units, need_dx, views, keep):
    def run():
        from sar_amd import ops
        N, C, T, V = 2, 3, 4, 5
        new = (lambda: cn4(C, N, T, V)) if views else (lambda: Z(N, C, T, V))
        params, features = [], V * C
        for u in units:
            params += [Z(features, u), Z(u)]
            features = u
        x = new()
        _, saved = ops.tattn_forward(x, params, out=new() if views else None)
        ops.tattn_backward(x, saved, params, new(), need_dx=need_dx, dx=new() if views else None, keep={} if keep else None)
    return run


def tattn_cases():
    for units, need_dx, views in itertools.product(((1,), (6, 4, 1)), (True, False), (False, True)):
        yield _name("tattn L%d" % len(units), need_dx and "dx", views and "views"), _tattn(units, need_dx, views, False)
    yield "tattn L3 dx keep", _tattn((6, 4, 1), True, False, True)


# ------------------------------------------------------------------------------------------------ AdaptiveAdjacency
def _adjattn(N, C, T, V, K, Ce, four_d, need_dx, need_dA):
    def run():
        from sar_amd import ops
        kernel = (lambda: Z(1, 1, C, K * Ce)) if four_d else (lambda: Z(C, K * Ce))
        X, tk, pk = rows(C, N * T * V), kernel(), kernel()
        _, saved = ops.adjattn_forward(X, N, T, V, Z(K, V, V), tk, pk, Z(K * Ce))
        ops.adjattn_backward(X, N, T, V, saved, tk, pk, Z(N, K, V, V), need_dx=need_dx, need_dA=need_dA)
    return run


def adjattn_cases():
    for four_d, need_dx, need_dA in itertools.product((True, False), (True, False), (True, False)):
        yield (_name("adjattn", "4-d" if four_d else "2-d", need_dx and "dx", need_dA and "dA"),
               _adjattn(2, 4, 3, 5, 3, 2, four_d, need_dx, need_dA))
    yield "adjattn two slabs", _adjattn(1, 4, 38, 25, 1, 27, True, True, True)      # 513 steps: the first size with two slabs


# ------------------------------------------------------------------------------------------------ the 1x1 product
C1, M1 = 6, 4


def _conv1x1(which, N, V, out=False, pro=False, epi=False):
    def run():
        from sar_amd import ops, _lib as L
        geo, n = ops.column_geometry(N, V), N * V
        X, dy, W = rows(C1, n), rows(M1, n, 8), Z(C1, M1)
        fold = dict(pro=(Z(C1), Z(C1)), pro_relu=True) if pro else {}
        if which == "fwd":
            if epi:      # the statistics epilogue into the caller's partials, as _mlp_forward asks for it
                nparts = ops.conv_gemm_nparts(Kc=C1, M=M1, **geo)
                fold.update(epi=L.SAR_EPI_STATS, partials_out=Z(2, M1, nparts, 2)[1])
            ops.conv1x1_fwd(X, W, Z(M1), geo, out=rows(M1, n, 12) if out else None, **fold)
        elif which == "wgrad":
            ops.conv1x1_wgrad(X, dy, geo, **fold)
        else:
            mask = {}
            if epi:      # the masked gradient through a folded BN + ReLU, as _mlp_backward asks for it
                npm = ops.conv_gemm_nparts(Kc=M1, M=C1, transposed=True, epi=L.SAR_EPI_MASK, **geo)
                mask = dict(epi=L.SAR_EPI_MASK, aux=X, aux_affine=(Z(C1), Z(C1)), aux_mean=Z(C1), partials_out=Z(2, C1, npm, 2)[1])
            ops.conv1x1_dgrad(dy, W, geo, out=rows(C1, n, 12) if out else None, **mask)
    return run


def conv1x1_cases():
    for N, V in ((2, 25), (3, 130), (2, 67)):      # column_geometry: V' = 25, 26 (5 frames), 1 (67 frames)
        yield "conv1x1 fwd %dx%d" % (N, V), _conv1x1("fwd", N, V)
    for out, pro, epi in itertools.product((False, True), (False, True), (False, True)):
        yield _name("conv1x1 fwd", pro and "pro", epi and "stats", out and "out"), _conv1x1("fwd", 2, 25, out, pro, epi)
    for pro in (False, True):
        yield _name("conv1x1 wgrad", pro and "pro"), _conv1x1("wgrad", 2, 25, pro=pro)
    for out, epi in itertools.product((False, True), (False, True)):
        yield _name("conv1x1 dgrad", epi and "masked", out and "out"), _conv1x1("dgrad", 2, 25, out, epi=epi)


# ------------------------------------------------------------------------------------------------ the modules
def _module(make, x_shape, A_shape=None, A_grad=True):
    """one training forward + backward; x and (A_grad) A ask for their gradients"""
    def run():
        layer = make()
        x = Z(*x_shape).requires_grad_()
        args = (x,) if A_shape is None else (x, Z(*A_shape).requires_grad_(A_grad))
        y = layer(*args, True)
        y = y[0] if isinstance(y, tuple) else y
        y.backward(torch.zeros_like(y))
    return run


def module_cases():
    from models import agcn, gcn, lstm_sampler, stgcn
    N, T, V = 2, 3, 5
    yield "module GraphConv", _module(lambda: gcn.GraphConv(4), (N, 3, V), (N, V, V))
    yield "module GraphConvTD dense", _module(lambda: gcn.GraphConvTD(4), (N, 4, T, V), (3, V, V))
    yield "module GraphIsoConvTD", _module(lambda: gcn.GraphIsoConvTD([4, 6]), (N, 4, T, V), (2, V, V))
    yield "module TemporalAttention", _module(lambda: stgcn.TemporalAttention([6, 4]), (N, 3, 4, V))
    yield "module AdaptiveGraphConv", _module(lambda: agcn.AdaptiveGraphConv(8), (N, 4, T, V), (3, V, V))
    yield "module TemporalSampler", _module(lambda: lstm_sampler.TemporalSampler([3], top_k=2), (N, 3, 4, V))


GROUPS = (("pgc pgpool", pg_cases), ("gpool", gpool_cases), ("tattn", tattn_cases), ("adjattn", adjattn_cases),
          ("conv1x1", conv1x1_cases), ("modules", module_cases))


def cases():
    """(group, name, function), in the fixture's order"""
    for group, gen in GROUPS:
        for name, fn in gen():
            yield group, name, fn


if __name__ == "__main__":
    G.write_fixture(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "layer_launch_abi.json"), COMMIT, cases, FULL,
                    "make_golden_layer_launch_abi")
