"""models/gcn.py: GraphConv, GraphConvTD and AdjGraphConv, and models/stgcn.py: SpatioTemporalGraphConv, as torch modules on the HIP
kernels -- output and every gradient against float64 references fed the layer's own parameters (tests/gcn_reference.py for GraphConv
and AdjGraphConv, oracle.stgcn.graph_conv_td / st_block for GraphConvTD and the block).  Bars: rel_err < 2e-5 for the three single
layers (a 1x1 product and one contraction; no gradient is left out), 1e-4 for the block (BatchNorm backward is in its chain: the bar
of tests/test_gpu_stgcn_model.py).  The block's only gradients left out are the convolution biases directly in front of a
BatchNorm -- sgcn.bias, tcn_bias, res_bias: exactly zero plus rounding noise, as tests/test_gpu_adjacency.py:97-98."""
import pytest
import torch

import gcn_reference as R
from graph.ntu_rgb_d import Graph
from models.gcn import AdjGraphConv, GraphConv, GraphConvTD
from models.stgcn import BLOCKS, SpatioTemporalGraphConv
from oracle import stgcn as O
from util import rel_err

pytestmark = pytest.mark.gpu
BAR = 2e-5
BLOCK_BAR = 1e-4
BIASES_BEFORE_A_BATCHNORM = ("sgcn.bias", "tcn_bias", "res_bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _randomize(layer, seed):
    """biases start at zero: move them (a zero bias hides a missing bias path)"""
    with torch.no_grad():
        layer.bias.copy_(0.2 * _randn(*layer.bias.shape, seed=seed))


def _compare(what, out, ref, got_grads, ref_grads, names, bar=BAR):
    errs = [("out", rel_err(out, ref))] + [(n, rel_err(g, r)) for n, g, r in zip(names, got_grads, ref_grads)]
    print(what + ": " + "  ".join("%s %.2e" % e for e in errs))
    assert max(e for _, e in errs) < bar, errs


def _graph_A(dev):
    return torch.from_numpy(Graph().A).float().contiguous().to(dev)


def test_graph_conv(dev):
    """(3, 16, 25) -> 24 filters with a dense per-sample adjacency: x, kernel, bias and A gradients"""
    x, A, dout = _randn(3, 16, 25, seed=1), _randn(3, 25, 25, seed=2), _randn(3, 24, 25, seed=3)
    layer = GraphConv(24)
    xg, Ag = x.to(dev).requires_grad_(True), A.to(dev).requires_grad_(True)
    out, A_out = layer(xg, Ag, True)
    assert A_out is Ag and tuple(layer.kernel.shape) == (1, 16, 24) and tuple(layer.bias.shape) == (24,)
    _randomize(layer, 4)
    out, _ = layer(xg, Ag, True)
    got = torch.autograd.grad(out, (xg, Ag, layer.kernel, layer.bias), dout.to(dev))
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (x, A, layer.kernel, layer.bias)]
    ref = R.graph_conv(*leaves)
    want = torch.autograd.grad(ref, leaves, dout.double())
    _compare("GraphConv", out, ref, got, want, ("dx", "dA", "dkernel", "dbias"))
    # A without a gradient: the same output, no dA launch
    out2, _ = layer(xg, A.to(dev), True)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("V", [512, 67])
def test_graph_conv_at_large_and_prime_joint_counts(dev, V):
    """V = 512 is what the layer is for (the 1x1 product sees the columns as 8 x 64); a prime V > 64 factorises as V x 1"""
    x, A, dout = _randn(2, 16, V, seed=30), _randn(2, V, V, seed=31), _randn(2, 24, V, seed=32)
    layer = GraphConv(24)
    xg, Ag = x.to(dev).requires_grad_(True), A.to(dev).requires_grad_(True)
    layer(xg, Ag, True)
    _randomize(layer, 33)
    out, _ = layer(xg, Ag, True)
    got = torch.autograd.grad(out, (xg, Ag, layer.kernel, layer.bias), dout.to(dev))
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (x, A, layer.kernel, layer.bias)]
    ref = R.graph_conv(*leaves)
    want = torch.autograd.grad(ref, leaves, dout.double())
    _compare("GraphConv V = %d" % V, out, ref, got, want, ("dx", "dA", "dkernel", "dbias"))


def _td_reference(layer, x, A, dout, with_A):
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (x, layer.kernel, layer.bias, A)]
    ref = O.graph_conv_td(*leaves)
    want = torch.autograd.grad(ref, leaves if with_A else leaves[:3], dout.double())
    return ref, want


def test_graph_conv_td_fused_and_dense_paths(dev):
    """(2, 16, 12, 25) -> 24 filters with Graph().A: the fixed adjacency takes the gather-list kernel, the same A with
    requires_grad the 1x1 product + dense contraction; both against the oracle, the two outputs against each other, dA checked"""
    x, dout = _randn(2, 16, 12, 25, seed=5), _randn(2, 24, 12, 25, seed=6)
    A = _graph_A(dev)
    layer = GraphConvTD(24)
    xg = x.to(dev).requires_grad_(True)
    layer(xg, A, True)
    assert tuple(layer.kernel.shape) == (1, 1, 16, 72) and tuple(layer.bias.shape) == (72,)
    _randomize(layer, 7)
    out_f, _ = layer(xg, A, True)
    assert type(out_f.grad_fn).__name__.startswith("_GraphConvTDFusedFn")
    got_f = torch.autograd.grad(out_f, (xg, layer.kernel, layer.bias), dout.to(dev))
    ref, want = _td_reference(layer, x, A, dout, True)
    _compare("GraphConvTD fused", out_f, ref, got_f, want[:3], ("dx", "dkernel", "dbias"))
    Ag = A.clone().requires_grad_(True)
    out_d, _ = layer(xg, Ag, True)
    assert type(out_d.grad_fn).__name__.startswith("_ConvContractFn")
    got_d = torch.autograd.grad(out_d, (xg, layer.kernel, layer.bias, Ag), dout.to(dev))
    _compare("GraphConvTD dense, Graph().A", out_d, ref, got_d, want, ("dx", "dkernel", "dbias", "dA"))
    assert rel_err(out_d, out_f) < BAR


def test_graph_conv_td_random_dense_adjacency(dev):
    x, dout, A = _randn(2, 16, 12, 25, seed=8), _randn(2, 24, 12, 25, seed=9), 0.3 * _randn(3, 25, 25, seed=10)
    layer = GraphConvTD(24)
    xg, Ad = x.to(dev).requires_grad_(True), A.to(dev)
    layer(xg, Ad, True)
    _randomize(layer, 11)
    out, _ = layer(xg, Ad, True)                       # no gradient asked for A, but too dense for the gather lists
    assert type(out.grad_fn).__name__.startswith("_ConvContractFn")
    got = torch.autograd.grad(out, (xg, layer.kernel, layer.bias), dout.to(dev))
    ref, want = _td_reference(layer, x, A, dout, False)
    _compare("GraphConvTD dense, random A", out, ref, got, want, ("dx", "dkernel", "dbias"))


def test_graph_conv_td_retables_an_edited_adjacency(dev):
    """the gather tables are cached on (address, version): an in-place edit of A must reach the next call"""
    x = _randn(2, 16, 12, 25, seed=12).to(dev)
    A = _graph_A(dev)
    layer = GraphConvTD(24)
    first, _ = layer(x, A, True)
    A.mul_(2.0)
    second, _ = layer(x, A, True)
    assert rel_err(second, 2.0 * first) < 1e-6


def test_adj_graph_conv(dev):
    x, dout = _randn(2, 16, 12, 25, seed=13), _randn(2, 24, 12, 25, seed=14)
    layer = AdjGraphConv(24, Graph().A + 0.05 * _randn(3, 25, 25, seed=15).double().numpy())
    xg = x.to(dev).requires_grad_(True)
    layer(xg, True)
    _randomize(layer, 16)
    assert "adjacency_matrix" in dict(layer.named_parameters())
    out = layer(xg, True)
    got = torch.autograd.grad(out, (xg, layer.adjacency_matrix, layer.kernel, layer.bias), dout.to(dev))
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (x, layer.adjacency_matrix, layer.kernel, layer.bias)]
    ref = R.adj_graph_conv(*leaves)
    want = torch.autograd.grad(ref, leaves, dout.double())
    _compare("AdjGraphConv", out, ref, got, want, ("dx", "dA", "dkernel", "dbias"))


def test_state_dict_round_trip_is_bitwise(dev):
    x3, A3 = _randn(3, 16, 25, seed=17).to(dev), _randn(3, 25, 25, seed=18).to(dev)
    x4 = _randn(2, 16, 12, 25, seed=19).to(dev)
    A = _graph_A(dev)
    pairs = [(GraphConv(24), GraphConv(24), lambda l: l(x3, A3, True)[0]),
             (GraphConvTD(24), GraphConvTD(24), lambda l: l(x4, A, True)[0]),
             (AdjGraphConv(24, Graph().A), AdjGraphConv(24, 0.5 * Graph().A), lambda l: l(x4, True))]
    for i, (src, dst, call) in enumerate(pairs):
        want = call(src)
        _randomize(src, 20 + i)
        want = call(src)
        dst.load_state_dict(src.state_dict())          # dst has never been called: built from the kernel's shape
        assert set(dst.state_dict()) == set(src.state_dict())
        assert torch.equal(call(dst), want)


def test_bad_arguments_raise_value_error(dev):
    x3, A3 = _randn(3, 16, 25, seed=21).to(dev), _randn(3, 25, 25, seed=22).to(dev)
    x4 = _randn(2, 16, 12, 25, seed=23).to(dev)
    A = _graph_A(dev)
    with pytest.raises(ValueError, match="ncw,nvw->ncv"):
        GraphConv(24, einsum="ncw,nvw->ncv")
    with pytest.raises(ValueError, match="nkctv,kwv->nctw"):
        GraphConvTD(24, einsum="nkctv,kwv->nctw")
    with pytest.raises(ValueError, match="nkctv,kwv->nctw"):
        AdjGraphConv(24, Graph().A, einsum="nkctv,kwv->nctw")
    with pytest.raises(ValueError):
        GraphConv(24)(x3.transpose(1, 2), A3, True)                  # not contiguous
    with pytest.raises(ValueError):
        GraphConv(24)(x3.cpu(), A3, True)
    with pytest.raises(ValueError):
        GraphConv(24)(x3, A3.cpu(), True)
    with pytest.raises(ValueError):
        GraphConvTD(24)(x4.permute(0, 1, 3, 2), A, True)
    with pytest.raises(ValueError):
        GraphConvTD(24)(x4.cpu(), A, True)
    with pytest.raises(ValueError):
        AdjGraphConv(24, Graph().A)(x4.cpu(), True)
    with pytest.raises(ValueError):
        GraphConv(24)(x3.double(), A3, True)


def test_a_gradient_that_is_not_asked_for_changes_no_other(dev):
    """backward launches only what needs_input_grad asks for: each gradient alone is bitwise the one of the full backward"""
    x, A, dout = _randn(3, 16, 25, seed=24).to(dev), _randn(3, 25, 25, seed=25).to(dev), _randn(3, 24, 25, seed=26).to(dev)
    layer = GraphConv(24)
    xg, Ag = x.clone().requires_grad_(True), A.clone().requires_grad_(True)
    full = torch.autograd.grad(layer(xg, Ag, True)[0], (xg, Ag, layer.kernel, layer.bias), dout)
    only_k, = torch.autograd.grad(layer(x, A, True)[0], (layer.kernel,), dout)
    only_x, = torch.autograd.grad(layer(xg, A, True)[0], (xg,), dout)
    layer.requires_grad_(False)
    only_A, = torch.autograd.grad(layer(x, Ag, True)[0], (Ag,), dout)
    assert torch.equal(only_A, full[1]) and torch.equal(only_k, full[2]) and torch.equal(only_x, full[0])
    x4, d4, G = _randn(2, 16, 12, 25, seed=27).to(dev), _randn(2, 24, 12, 25, seed=28).to(dev), _graph_A(dev)
    for A4 in (G, G.clone().requires_grad_(True)):                 # the fused and the dense path
        td = GraphConvTD(24)
        x4g = x4.clone().requires_grad_(True)
        full = torch.autograd.grad(td(x4g, A4, True)[0], (x4g, td.kernel, td.bias), d4)
        only_b, = torch.autograd.grad(td(x4, A4, True)[0], (td.bias,), d4)
        td.requires_grad_(False)
        only_x, = torch.autograd.grad(td(x4g, A4, True)[0], (x4g,), d4)
        assert torch.equal(only_x, full[0]) and torch.equal(only_b, full[2])
        if A4.requires_grad:
            ref_A, = torch.autograd.grad(td(x4g, A4, True)[0], (A4,), d4)
            only_A, = torch.autograd.grad(td(x4, A4, True)[0], (A4,), d4)
            assert torch.equal(only_A, ref_A)


# ------------------------------------------------------------------------------------------------ SpatioTemporalGraphConv
def _built_block(dev, cin, f, s, res, T, seed):
    """a block built by one call, its affine parameters and biases moved off their (1, 0) start, its moving statistics reset"""
    layer = SpatioTemporalGraphConv(f, stride=s, residual=res)
    x = _randn(2, cin, T, 25, seed=seed)
    layer(x.to(dev), _graph_A(dev), True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in layer.named_parameters():
            if not k.endswith("kernel"):
                v.add_(0.2 * torch.randn(v.shape, generator=g).to(dev))
        for k, b in layer.named_buffers():
            b.fill_(1.0 if k.endswith("var") else 0.0)
    return layer, x


def _block_against_the_oracle(dev, cin, f, s, res, T, seed, kind, A_grad=False):
    layer, x = _built_block(dev, cin, f, s, res, T, seed)
    assert layer.kind == kind
    blocks = [(f, s, res)]
    p = R.block_params(layer)
    A = _graph_A(dev).requires_grad_(A_grad)
    xg = x.to(dev).requires_grad_(True)
    out, A_out = layer(xg, A, True)
    assert A_out is A
    To = -(-T // s)
    assert tuple(out.shape) == (2, f, To, 25)
    dout = _randn(2, f, To, 25, seed=seed + 2)
    names = [k for k, _ in layer.named_parameters()]
    got = torch.autograd.grad(out, [xg] + [v for _, v in layer.named_parameters()] + ([A] if A_grad else []), dout.to(dev))
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if "moving" not in k}
    q = dict(p)
    q.update(leaves)
    xd, Ad = x.double().requires_grad_(True), A.detach().double().cpu().requires_grad_(True)
    new_stats = {}
    ref = O.st_block(xd, q, 0, Ad, True, new_stats, blocks=blocks)
    pnames = [R.oracle_name(n) for n in names]   # each gradient is compared with that of the oracle's leaf of ITS OWN name
    assert len(set(pnames)) == len(names) and set(pnames) == set(leaves)
    for n, o in zip(names, pnames):
        assert torch.equal(dict(layer.named_parameters())[n].detach().double().cpu(), leaves[o].detach()), (n, o)
    want = torch.autograd.grad(ref, [xd] + [leaves[n] for n in pnames] + ([Ad] if A_grad else []), dout.double())
    keep = [0] + [1 + i for i, n in enumerate(names) if n not in BIASES_BEFORE_A_BATCHNORM] + ([len(names) + 1] if A_grad else [])
    label = ["dx"] + names + ["dA"]
    _compare("block %s" % kind + (" dense A" if A_grad else ""), out, ref, [got[i] for i in keep], [want[i] for i in keep],
             [label[i] for i in keep], bar=BLOCK_BAR)
    after = R.block_params(layer)
    for k, v in new_stats.items():               # the moving statistics moved as the oracle's (momentum 0.99, unbiased variance)
        assert rel_err(after[k], v) < 1e-5, k
    return layer, x


def test_block_stride_1_identity_residual(dev):
    _block_against_the_oracle(dev, 16, 16, 1, True, 20, 40, "identity")


def test_block_stride_2_convolutional_residual_odd_frames(dev):
    """T = 21: SAME padding (3, 4) of the strided temporal convolution and the strided residual's frame selection"""
    _block_against_the_oracle(dev, 16, 32, 2, True, 21, 50, "conv")


def test_block_without_residual(dev):
    _block_against_the_oracle(dev, 16, 16, 1, False, 20, 60, "none")


def test_block_with_a_trainable_adjacency_gives_dA(dev):
    _block_against_the_oracle(dev, 16, 32, 2, True, 21, 70, "conv", A_grad=True)


def test_block_inference_uses_the_moving_statistics_and_leaves_them(dev):
    layer, x = _built_block(dev, 16, 32, 2, True, 21, 80)
    A = _graph_A(dev)
    for _ in range(2):
        layer(x.to(dev), A, True)
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    assert not torch.equal(before["bn1_moving_mean"], torch.zeros_like(before["bn1_moving_mean"]))
    out, _ = layer(x.to(dev), A, False)
    ref = O.st_block(x.double(), R.block_params(layer), 0, A.double().cpu(), False, blocks=[(32, 2, True)])
    print("block inference: out %.2e" % rel_err(out, ref))
    assert rel_err(out, ref) < BLOCK_BAR
    assert all(torch.equal(v, before[k]) for k, v in layer.state_dict().items())
    layer.eval()                                  # training=None follows the module's mode
    assert torch.equal(layer(x.to(dev), A)[0], out)


def test_block_state_dict_round_trip_and_bad_arguments(dev):
    layer, x = _built_block(dev, 16, 32, 2, True, 21, 90)
    A = _graph_A(dev)
    layer(x.to(dev), A, True)
    fresh = SpatioTemporalGraphConv(32, stride=2)
    fresh.load_state_dict(layer.state_dict())
    assert fresh.kind == "conv" and set(fresh.state_dict()) == set(layer.state_dict())
    assert torch.equal(fresh(x.to(dev), A, False)[0], layer(x.to(dev), A, False)[0])
    assert torch.equal(fresh(x.to(dev), A, True)[0], layer(x.to(dev), A, True)[0])
    with pytest.raises(ValueError, match="tanh"):
        SpatioTemporalGraphConv(32, activation="tanh")
    with pytest.raises(ValueError):
        SpatioTemporalGraphConv(32, kernel_size=[3, 5])
    with pytest.raises(ValueError):
        layer(x, A, True)                          # CPU tensor
    with pytest.raises(ValueError):
        layer(x.to(dev).permute(0, 1, 3, 2), A, True)


def test_ten_block_body_trains(dev):
    """the snippet of INTEGRATION.md: the reference's ten-block body from layers and Graph().A, two steps of a torch optimizer at
    batch 2; the loss is finite and every parameter moves"""
    torch.manual_seed(0)
    A = _graph_A(dev)
    body = torch.nn.ModuleList(SpatioTemporalGraphConv(f, stride=s, residual=r) for f, s, r in BLOCKS)
    head = torch.nn.Linear(256, 60).to(dev)
    x, labels = _randn(2, 3, 64, 25, seed=99).to(dev), torch.tensor([3, 7], device=dev)
    h = x
    for blk in body:
        h, _ = blk(h, A, True)
    assert tuple(h.shape) == (2, 256, 16, 25)
    assert [b.kind for b in body] == ["none", "identity", "identity", "identity", "conv", "identity", "identity", "conv", "identity", "identity"]
    opt = torch.optim.SGD(list(body.parameters()) + list(head.parameters()), lr=0.01, momentum=0.9, nesterov=True)
    start = {k: v.detach().clone() for k, v in body.named_parameters()}
    losses = []
    for step in range(2):
        h = x
        for blk in body:
            h, _ = blk(h, A, True)
        loss = torch.nn.functional.cross_entropy(head(h.mean(dim=(2, 3))), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("ten-block body: loss %.4f -> %.4f" % tuple(losses))
    assert all(torch.isfinite(torch.tensor(losses)))
    # every parameter moved, by name; only the biases in front of a BatchNorm (zero gradient plus rounding noise) are not asked
    still = [k for k, v in body.named_parameters()
             if k.split(".", 1)[1] not in BIASES_BEFORE_A_BATCHNORM and torch.equal(v.detach(), start[k])]
    assert len(start) == 10 * 8 + 2 * 4 and not still, still
