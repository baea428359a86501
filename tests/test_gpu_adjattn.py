"""GPU: AdaptiveAdjacency (csrc/adjattn.hip through the C ABI, sar_amd.ops, and the modules of models/agcn.py) against the float64
restatement tests/adjattn_reference.py over the cases of tests/adjattn_cases.py.

Each of the four kernels runs on its own, its inputs the float64 reference's intermediates rounded to float32, and is judged against
float64; then the whole layer runs through ops and through the module (A_eff, dx, dtheta.kernel, dphi.kernel, dphi.bias, dA), and
AdaptiveGraphConv against the same restatement composed with tests/gpool_reference.sgcn_forward under float64 autograd.

Tolerance (the rule of tests/test_gpu_tattn.py): norm-wise relative error (tests/util.rel_err) below TOL = 2e-5; a quantity that misses TOL
is judged against 8x the distance of the float32 run of the SAME restatement (CPU) from float64.  Both numbers are printed.

Worst errors observed on MI355X per quantity: profiles/adjattn.txt."""
import pytest
import torch

import adjattn_cases as K
import adjattn_reference as R
import gpool_reference as G
from util import rel_err, to_cn

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def judge(name, got, ref64, ref32):
    e, band = rel_err(got, ref64), rel_err(ref32, ref64)
    print("%-14s engine %.3e, float32 restatement %.3e from float64" % (name, e, band))
    return None if (e < TOL or e <= 8 * band) else (e, band)


def assert_all(pairs):
    bad = {k: v for k, v in pairs.items() if v is not None}
    assert not bad, "(engine error, float32 band) beyond TOL and 8x the band: %s" % bad


def f32(t, dev):
    return t.to(torch.float32).to(dev).contiguous()


def keras(kernel):
    """(C, K Ce) -> the Keras layout (1, 1, C, K Ce)"""
    return kernel.reshape(1, 1, *kernel.shape)


def kernels(dev, case):
    """the four entry points one at a time on the float64 reference's intermediates rounded to float32 -> dict of their results"""
    from sar_amd import _lib as L
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, T, V, Kk, Ce, _ = case
    (x, A, tk, pk, pb, dA_eff), r64, _ = K.reference(case)
    lib, st, n, kce = L.load(), stream_ptr(), N * T * V, Kk * Ce
    E = f32(torch.cat([to_cn(r64["theta"]), to_cn(r64["phi"])]), dev)
    Ad, S64, P64, dd, dS64 = f32(A, dev), f32(r64["S"], dev), f32(r64["P"], dev), f32(dA_eff, dev), f32(r64["dS"], dev)

    def new(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    S, P, A_eff, dS, dA, dE = new(N, Kk, V, V), new(N, Kk, V, V), new(N, Kk, V, V), new(N, Kk, V, V), new(Kk, V, V), new(2 * kce, n)
    nslab = lib.sar_adjattn_sim_slabs(Ce, T, V)
    slab = new(nslab, N * Kk * V * V) if nslab > 1 else None
    check(lib.sar_adjattn_sim_f32(ptr(E), ptr(E[kce:]), n, N, Kk, Ce, T, V, ptr(S), ptr(slab), nslab, st), "sim")
    check(lib.sar_adjattn_softmax_f32(ptr(S64), ptr(Ad), N, Kk, V, ptr(P), ptr(A_eff), st), "softmax")
    check(lib.sar_adjattn_softmax_bwd_f32(ptr(P64), ptr(dd), N, Kk, V, ptr(dS), ptr(dA), st), "softmax_bwd")
    check(lib.sar_adjattn_dembed_f32(ptr(dS64), ptr(E), ptr(E[kce:]), n, N, Kk, Ce, T, V, ptr(dE), ptr(dE[kce:]), n, st), "dembed")
    torch.cuda.synchronize()
    return dict(S=S, P=P, A_eff=A_eff, dS=dS, dA=dA, dtheta=dE[:kce], dphi=dE[kce:])


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_each_kernel_matches_the_float64_restatement(dev, case):
    _, r64, r32 = K.reference(case)
    got = kernels(dev, case)
    want = lambda r: dict(S=r["S"], P=r["P"], A_eff=r["A_eff"], dS=r["dS"], dA=r["dA"], dtheta=to_cn(r["dtheta"]), dphi=to_cn(r["dphi"]))
    w64, w32 = want(r64), want(r32)
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), "an element was not written"
    assert_all({k: judge(k, got[k], w64[k], w32[k]) for k in w64})


def run_ops(dev, case, need_dx=True, need_dA=True):
    from sar_amd import ops
    N, C, T, V = case[:4]
    (x, A, tk, pk, pb, dA_eff), _, _ = K.reference(case)
    X, tkd, pkd = f32(to_cn(x), dev), f32(keras(tk), dev), f32(keras(pk), dev)
    A_eff, saved = ops.adjattn_forward(X, N, T, V, f32(A, dev), tkd, pkd, f32(pb, dev))
    dX, dtk, dpk, dpb, dA = ops.adjattn_backward(X, N, T, V, saved, tkd, pkd, f32(dA_eff, dev), need_dx=need_dx, need_dA=need_dA)
    torch.cuda.synchronize()
    return dict(A_eff=A_eff, P=saved[1], dx=dX, dtheta_kernel=dtk, dphi_kernel=dpk, dphi_bias=dpb, dA=dA)


def judge_layer(got, r64, r32, shape):
    N, C, T, V = shape
    pairs = {}
    for q in K.QUANTITIES:
        g = got[q]
        if q == "dx" and g.dim() == 2:
            g = g.view(C, N, T, V).permute(1, 0, 2, 3)
        pairs[q] = judge(q, g.reshape(r64[q].shape), r64[q], r32[q])
    assert_all(pairs)


def assert_one_vertex(got):
    """V = 1: P = 1 and exactly zero dx, dtheta.kernel, dphi.kernel, dphi.bias"""
    for q in ("dx", "dtheta_kernel", "dphi_kernel", "dphi_bias"):
        assert torch.equal(got[q], torch.zeros_like(got[q])), q


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_layer_through_ops_matches_the_float64_restatement(dev, case):
    _, r64, r32 = K.reference(case)
    got = run_ops(dev, case)
    judge_layer(got, r64, r32, case[:4])
    if case[3] == 1:
        assert torch.equal(got["P"], torch.ones_like(got["P"]))
        assert_one_vertex(got)


def make_module(dev, case):
    from models.agcn import AdaptiveAdjacency
    (x, A, tk, pk, pb, dA_eff), _, _ = K.reference(case)
    m = AdaptiveAdjacency(case[5], case[4])
    m.load_state_dict({"theta.kernel": f32(keras(tk), dev), "phi.kernel": f32(keras(pk), dev), "phi.bias": f32(pb, dev)})
    return m, f32(x, dev), f32(A, dev), f32(dA_eff, dev)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_module_matches_the_float64_restatement(dev, case):
    _, r64, r32 = K.reference(case)
    m, xd, Ad, dd = make_module(dev, case)
    xd.requires_grad_()
    Ad.requires_grad_()
    A_eff = m(xd, Ad, True)
    A_eff.backward(dd)
    torch.cuda.synchronize()
    got = dict(A_eff=A_eff.detach(), dx=xd.grad, dtheta_kernel=m.theta.kernel.grad, dphi_kernel=m.phi.kernel.grad, dphi_bias=m.phi.bias.grad,
               dA=Ad.grad)
    judge_layer(got, r64, r32, case[:4])
    if case[3] == 1:
        assert_one_vertex(got)


@pytest.mark.parametrize("case", [K.LISTED[0], K.LISTED[7], K.EDGES[0]], ids=K.case_id)
def test_two_runs_are_bitwise_equal(dev, case):
    a, b = run_ops(dev, case), run_ops(dev, case)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_need_dx_false_and_need_dA_false_change_nothing_else(dev):
    case = K.LISTED[1]
    a = run_ops(dev, case)
    for flags in (dict(need_dx=False), dict(need_dA=False), dict(need_dx=False, need_dA=False)):
        b = run_ops(dev, case, **flags)
        assert (b["dx"] is None) == ("need_dx" in flags) and (b["dA"] is None) == ("need_dA" in flags)
        for k in a:
            assert b[k] is None or torch.equal(a[k], b[k]), (k, flags)


def test_a_sample_does_not_depend_on_the_rest_of_the_batch(dev):
    """every 4-sample slice of the 16-sample run is bitwise the N = 4 run on that slice; the slice of X is a row-strided view (ld = the
    16 samples' columns).  Parameter gradients and dA are batch sums and are not compared"""
    from sar_amd import ops
    N, C, T, V = K.SLICE[:4]
    (x, A, tk, pk, pb, dA_eff), _, _ = K.reference(K.SLICE)
    X, Ad, tkd, pkd, pbd, dd = f32(to_cn(x), dev), f32(A, dev), f32(keras(tk), dev), f32(keras(pk), dev), f32(pb, dev), f32(dA_eff, dev)
    A_eff, saved = ops.adjattn_forward(X, N, T, V, Ad, tkd, pkd, pbd)
    dX = ops.adjattn_backward(X, N, T, V, saved, tkd, pkd, dd)[0]
    n4 = K.SLICE_N
    for n0 in range(0, N, n4):
        cols = slice(n0 * T * V, (n0 + n4) * T * V)
        Xs = X[:, cols]
        a4, s4 = ops.adjattn_forward(Xs, n4, T, V, Ad, tkd, pkd, pbd)
        d4 = ops.adjattn_backward(Xs, n4, T, V, s4, tkd, pkd, dd[n0:n0 + n4].contiguous())[0]
        assert torch.equal(a4, A_eff[n0:n0 + n4]), "A_eff, samples %d.." % n0
        assert torch.equal(s4[1], saved[1][n0:n0 + n4]), "P, samples %d.." % n0
        assert torch.equal(s4[0], saved[0][:, cols]), "theta | phi, samples %d.." % n0
        assert torch.equal(d4, dX[:, cols]), "dX, samples %d.." % n0


def test_module_creates_its_parameters_lazily_in_the_keras_layouts(dev):
    from models.agcn import AdaptiveAdjacency
    N, C, T, V, Kk, Ce = 2, 64, 9, 25, 3, 16
    m = AdaptiveAdjacency(Ce)
    assert list(m.parameters()) == []
    torch.manual_seed(0)
    A = torch.rand(Kk, V, V, device=dev)
    A_eff = m(torch.randn(N, C, T, V, device=dev), A)
    assert tuple(A_eff.shape) == (N, Kk, V, V)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [("theta.kernel", (1, 1, C, Kk * Ce)), ("phi.kernel", (1, 1, C, Kk * Ce)),
                                                                      ("phi.bias", (Kk * Ce,))]
    std = (2.0 / (Kk * Ce)) ** 0.5                                        # VarianceScaling(2, fan_out, truncated_normal)
    for k in (m.theta.kernel.detach(), m.phi.kernel.detach()):
        assert k.is_cuda and abs(float(k.std()) - std) < 0.1 * std and float(k.abs().max()) <= 2 * std / .87962566103423978 + 1e-6
    assert not bool(m.phi.bias.detach().any())
    assert float(((A_eff.detach() - A).sum(dim=2) - 1).abs().max()) < 1e-4        # every column of P sums to 1
    with pytest.raises(ValueError, match="input channels"):
        m(torch.randn(N, C + 1, T, V, device=dev), torch.rand(Kk, V, V, device=dev))


def test_module_round_trips_a_state_dict(dev):
    from models.agcn import AdaptiveAdjacency
    case = K.LISTED[0]
    m, xd, Ad, _ = make_module(dev, case)
    want = m(xd, Ad)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(state) == ["phi.bias", "phi.kernel", "theta.kernel"]
    m2 = AdaptiveAdjacency(case[5], case[4])
    m2.load_state_dict(state)
    assert torch.equal(m2(xd, Ad), want)


def test_module_saves_nothing_under_no_grad(dev):
    m, xd, Ad, _ = make_module(dev, K.LISTED[0])
    with torch.no_grad():
        out = m(xd, Ad, True)
    assert out.grad_fn is None and not out.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    out = m(xd, Ad, True)                                    # nothing requires a gradient
    assert out.grad_fn is None and not out.requires_grad
    Ad.requires_grad_()                                      # a trainable A + B alone asks for the node
    out = m(xd, Ad, True)
    out.sum().backward()
    assert torch.equal(Ad.grad, torch.full_like(Ad, float(xd.shape[0]))) and xd.grad is None
    Ad.requires_grad_(False)
    for p in m.parameters():
        p.requires_grad_(True)
    seen = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t) or t, lambda t: t):
        with torch.no_grad():
            m(xd, Ad, True)
        assert seen == []
        m(xd, Ad, True)
    assert len(seen) == 5                                    # X, theta | phi, P and the two kernels


def test_modules_reject_what_they_are_not_built_for(dev):
    from models.agcn import AdaptiveAdjacency, AdaptiveGraphConv
    x, A = torch.randn(2, 4, 6, 5, device=dev), torch.rand(3, 5, 5, device=dev)
    for m in (AdaptiveAdjacency(2), AdaptiveGraphConv(8)):
        for bx, bA in ((x.double(), A), (x[:, :, ::2], A), (x.cpu(), A), (x[0], A), (x[:0], A), (x, A.double()), (x, A[:2]), (x, A[:, :4]),
                       (x, A.expand(2, 3, 5, 5).contiguous()), (x, A.transpose(1, 2)), (torch.randn(2, 4, 6, 33, device=dev), torch.rand(3, 33, 33, device=dev))):
            with pytest.raises(ValueError):
                m(bx, bA, True)
        assert list(m.parameters()) == [], "a rejected call built or launched something"
    g = AdaptiveGraphConv(8, kernel_size=3)
    with pytest.raises(ValueError, match="K \\* V <= 76"):              # SGCN's limit: 3 * 26 = 78
        g(torch.randn(2, 4, 6, 26, device=dev), torch.rand(3, 26, 26, device=dev))
    assert list(g.parameters()) == []


# ---- AdaptiveGraphConv: AdaptiveAdjacency -> SGCN, two autograd nodes
GCONV_FILTERS = 6


def gconv_case(case):
    """the case's inputs plus SGCN's kernel (1, 1, C, K F), bias (K F) and dy (N, F, T, V), float64"""
    N, C, T, V, Kk, Ce, seed = case
    gen = torch.Generator().manual_seed(seed + 100)
    r = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64)
    return K.make_case(case)[:5] + (r((1, 1, C, Kk * GCONV_FILTERS)) / C ** 0.5, 0.1 * r((Kk * GCONV_FILTERS,)), r((N, GCONV_FILTERS, T, V)))


def gconv_reference(inputs, dtype):
    x, A, tk, pk, pb, gk, gb, dy = (t.to(dtype) for t in inputs)
    leaves = [t.clone().requires_grad_() for t in (x, A, tk, pk, pb, gk, gb)]
    y = G.sgcn_forward(leaves[0], R.literal(*leaves[:5]), leaves[5], leaves[6])
    return [y.detach()] + list(torch.autograd.grad(y, leaves, dy))


GCONV_NAMES = ("y", "dx", "dA", "dtheta.kernel", "dphi.kernel", "dphi.bias", "dgcn.kernel", "dgcn.bias")


def make_gconv(dev, case, inputs):
    from models.agcn import AdaptiveGraphConv
    x, A, tk, pk, pb, gk, gb, dy = inputs
    m = AdaptiveGraphConv(GCONV_FILTERS, case[4], case[5])
    m.load_state_dict({"adjacency.theta.kernel": f32(keras(tk), dev), "adjacency.phi.kernel": f32(keras(pk), dev), "adjacency.phi.bias": f32(pb, dev),
                       "gcn.kernel": f32(gk, dev), "gcn.bias": f32(gb, dev)})
    return m


@pytest.mark.parametrize("case", K.LISTED[:2], ids=K.case_id)
def test_adaptive_graph_conv_matches_the_composed_float64_restatement(dev, case):
    inputs = gconv_case(case)
    w64, w32 = gconv_reference(inputs, torch.float64), gconv_reference(inputs, torch.float32)
    m = make_gconv(dev, case, inputs)
    xd, Ad, dy = f32(inputs[0], dev).requires_grad_(), f32(inputs[1], dev).requires_grad_(), f32(inputs[7], dev)
    y, A_out = m(xd, Ad, True)
    assert A_out is Ad and tuple(y.shape) == tuple(dy.shape)
    y.backward(dy)
    torch.cuda.synchronize()
    a = m.adjacency
    got = [y.detach(), xd.grad, Ad.grad, a.theta.kernel.grad, a.phi.kernel.grad, a.phi.bias.grad, m.gcn.kernel.grad, m.gcn.bias.grad]
    assert_all({n: judge(n, g.reshape(r64.shape), r64, r32) for n, g, r64, r32 in zip(GCONV_NAMES, got, w64, w32)})


def test_three_sgd_steps_of_adaptive_graph_conv_lower_the_loss(dev):
    case = K.LISTED[0]
    inputs = gconv_case(case)
    m = make_gconv(dev, case, inputs)
    xd, Ad, target = f32(inputs[0], dev), f32(inputs[1], dev), f32(inputs[7], dev)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    before = [p.detach().clone() for p in m.parameters()]
    losses = []
    for _ in range(4):
        loss = ((m(xd, Ad, True)[0] - target) ** 2).mean()
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("losses: %s" % losses)
    assert losses[3] < losses[0]
    assert len(before) == 5 and all(not torch.equal(p.detach(), old) for p, old in zip(m.parameters(), before))
