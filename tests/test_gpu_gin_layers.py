"""models/gcn.py: GraphIsoConv and GraphIsoConvTD as torch modules on the HIP kernels -- output and every gradient against the float64
restatements of tests/gin_reference.py fed the layer's own parameters.

Bar: rel_err < 1e-4 (BatchNorm backward is in the chain: BLOCK_BAR of tests/test_gpu_layers.py); float32 torch stays at or below 2e-6
on these shapes.  Biases, gamma, beta and epsilon (0.3) are moved off their (0, 1, 0, 0) start before comparing, so that a missing
path shows.  The only gradients left out are the convolution biases directly in front of a BatchNorm (exactly zero plus rounding
noise, as BIASES_BEFORE_A_BATCHNORM there); with return_logits=True the last bias is compared.  Every case asserts on the float64
reference that no pre-ReLU value lies within 1e-5 of zero, so that a flipped ReLU mask cannot pass for an arithmetic error: the
seeds below were chosen for that on the CPU (the layer's parameters are drawn on the host, so the reference does not depend on
the GPU).

GraphIsoConvTD's d epsilon is compared like every other gradient, and it is the ill-conditioned one: the self slice (1 + eps) x feeds
Conv -> BatchNorm, which cancels the scale of its input up to the BatchNorm's eps, so the float64 gradient is about 1e-3 of the terms
that add up to it (3.3e-4 .. 4.2e-3 in the first four cases here).  Float32 torch autograd on the CPU misses it by 3.3e-3, 6.5e-3, 3.8e-3
and 7.8e-2 in these cases, and so did the layer (4.1e-3, 2.4e-3, 5.3e-4, 7.6e-2) while it took d epsilon as the trace of the table
gradient's self slice; the closed form from the first BatchNorm's backward (sar_gin_eps_grad_bn_f32) is what meets the bar."""
import pytest
import torch

import gin_reference as R
from graph.ntu_rgb_d import Graph
from models.gcn import GraphIsoConv, GraphIsoConvTD
from util import rel_err

pytestmark = pytest.mark.gpu
BAR = 1e-4
MARGIN = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def built(layer, cin, device, seed):
    """the layer's parameters created as the first call creates them, then moved off their start: kernels as initialised (host
    generator seeded here), biases / gamma / beta shifted by 0.2 randn, epsilon = 0.3"""
    torch.manual_seed(seed)
    layer.build(cin, device)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in layer.named_parameters():
            if k == "epsilon":
                v.fill_(0.3)
            elif not k.endswith("kernel"):
                v.add_(0.2 * torch.randn(v.shape, generator=g).to(v.device))
    return layer


def compared(layer):
    """parameter names whose gradient is compared: all but the biases in front of a BatchNorm"""
    names = [k for k, _ in layer.named_parameters()]
    return [k for k in names if not (k.endswith(".bias") and k[:-4] + "gamma" in names)]


def reference(layer, x, A, dout, A_grad, training=True):
    """float64 output, gradients {name: tensor} (x, A when asked, every parameter), the moving statistics after the call and the
    smallest |pre-ReLU value|"""
    p = R.layer_params(layer)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if "moving" not in k}
    q = dict(p)
    q.update(leaves)
    xd, Ad = x.double().requires_grad_(True), A.detach().double().cpu().requires_grad_(A_grad)
    stats, pre = {}, []
    if isinstance(layer, GraphIsoConvTD):
        ref = R.graph_iso_conv_td(xd, Ad, q, layer.filters, layer.kernel_size, training=training, new_stats=stats, pre_relu=pre)
    else:
        ref = R.graph_iso_conv(xd, Ad, q, layer.filters, layer.return_logits, training=training, new_stats=stats, pre_relu=pre)
    grads = {}
    if training:
        names = list(leaves)
        got = torch.autograd.grad(ref, [xd] + [leaves[k] for k in names] + ([Ad] if A_grad else []), dout.double())
        grads = dict(zip(["x"] + names + (["A"] if A_grad else []), got))
    margin = min(t.abs().min().item() for t in pre) if pre else float("inf")
    return ref.detach(), grads, stats, margin


def against_the_reference(dev, what, layer, x, A, dout, A_grad):
    xg, Ag = x.to(dev).requires_grad_(True), A.to(dev).contiguous().requires_grad_(A_grad)
    before = R.layer_params(layer)
    ref, want, stats, margin = reference(layer, x, A, dout, A_grad)
    assert margin > MARGIN, "%s: a pre-ReLU value of the reference lies %.2e from zero: choose another seed" % (what, margin)
    out, A_out = layer(xg, Ag, True)
    assert A_out is Ag and tuple(out.shape) == tuple(ref.shape)
    names = compared(layer)
    params = dict(layer.named_parameters())
    got = torch.autograd.grad(out, [xg] + [params[k] for k in names] + ([Ag] if A_grad else []), dout.to(dev))
    labels = ["x"] + names + (["A"] if A_grad else [])
    errs = [("out", rel_err(out, ref))] + [(k, rel_err(g, want[k])) for k, g in zip(labels, got)]
    print("%s (pre-ReLU margin %.1e): " % (what, margin) + "  ".join("%s %.2e" % e for e in errs))
    assert all(tuple(g.shape) == tuple(want[k].shape) for k, g in zip(labels, got))
    assert max(e for _, e in errs) < BAR, errs
    after = R.layer_params(layer)
    assert set(stats) == {k for k in after if "moving" in k}
    for k, v in stats.items():                   # the moving statistics moved as the reference's
        assert not torch.equal(after[k], before[k]) and rel_err(after[k], v) < 1e-5, k
    # A without a gradient: the same output
    out2, _ = layer(x.to(dev), A.to(dev).contiguous(), True)
    assert torch.equal(out2, out)
    return out


ISO_CASES = {"two layers, dA": ([32, 24], False, (3, 16, 25), True, 101),
             "prime V = 67": ([24], False, (2, 16, 67), False, 111),
             "logits, V = 130": ([16, 16, 8], True, (4, 8, 130), False, 120),
             "V = 512": ([24], False, (2, 16, 512), False, 130)}


def iso_case(name, device):
    filters, logits, (N, C, V), A_grad, seed = ISO_CASES[name]
    layer = built(GraphIsoConv(filters, return_logits=logits), C, device, seed)
    x, A, dout = _randn(N, C, V, seed=seed + 2), _randn(N, V, V, seed=seed + 3) / V ** 0.5, _randn(N, filters[-1], V, seed=seed + 4)
    return layer, x, A, dout, A_grad


@pytest.mark.parametrize("name", list(ISO_CASES))
def test_graph_iso_conv(dev, name):
    against_the_reference(dev, "GraphIsoConv " + name, *iso_case(name, dev))


# the last three: cin != f in the second MLP layer (a swapped cin / f in a stacked-row view, a partials shape or a weight stride shows),
# depth 1 and depth 3
TD_CASES = {"Graph().A[1:]": ([12, 12], 3, "graph", False, 200), "random A, dA": ([12, 12], 3, "random", True, 219),
            "kernel_size 2": ([12, 12], 2, "random", False, 221), "kernel_size 4": ([12, 12], 4, "random", True, 231),
            "unequal widths": ([12, 8], 3, "random", True, 261), "one layer": ([8], 2, "random", False, 240),
            "three layers": ([12, 8, 20], 2, "random", True, 240)}


def td_case(name, device):
    filters, K, kind, A_grad, seed = TD_CASES[name]
    layer = built(GraphIsoConvTD(filters, kernel_size=K), 16, device, seed)
    x, dout = _randn(2, 16, 12, 25, seed=seed + 2), _randn(2, filters[-1], 12, 25, seed=seed + 4)
    A = torch.from_numpy(Graph().A[1:]).float() if kind == "graph" else 0.3 * _randn(K - 1, 25, 25, seed=seed + 3)
    return layer, x, A, dout, A_grad


@pytest.mark.parametrize("name", list(TD_CASES))
def test_graph_iso_conv_td(dev, name):
    against_the_reference(dev, "GraphIsoConvTD " + name, *td_case(name, dev))


def test_parameters_are_created_on_the_first_call_with_the_keras_names(dev):
    layer = GraphIsoConv([32, 24], return_logits=True)
    assert not list(layer.parameters())
    layer(_randn(3, 16, 25, seed=1).to(dev), _randn(3, 25, 25, seed=2).to(dev), True)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {
        "epsilon": (), "mlp.0.kernel": (1, 16, 32), "mlp.0.bias": (32,), "mlp.0.gamma": (32,), "mlp.0.beta": (32,),
        "mlp.0.moving_mean": (32,), "mlp.0.moving_var": (32,), "mlp.1.kernel": (1, 32, 24), "mlp.1.bias": (24,)}
    assert sorted(k for k, _ in layer.named_buffers()) == ["mlp.0.moving_mean", "mlp.0.moving_var"]
    assert layer.epsilon.item() == 0.0 and not bool(layer.mlp[0].bias.any()) and bool((layer.mlp[0].gamma == 1).all())
    td = GraphIsoConvTD([12, 8], kernel_size=2)
    td(_randn(2, 16, 4, 25, seed=3).to(dev), _randn(1, 25, 25, seed=4).to(dev), True)
    want = {"epsilon": ()}
    for k in range(2):
        for i, (cin, f) in enumerate(((16, 12), (12, 8))):
            q = "mlps.%d.%d." % (k, i)
            want.update({q + "kernel": (1, 1, cin, f), q + "bias": (f,), q + "gamma": (f,), q + "beta": (f,), q + "moving_mean": (f,),
                         q + "moving_var": (f,)})
    assert {k: tuple(v.shape) for k, v in td.state_dict().items()} == want
    assert len(list(td.named_buffers())) == 8


def test_state_dict_round_trip_is_bitwise(dev):
    for name, make, case in (("two layers, dA", lambda: GraphIsoConv([32, 24]), iso_case),
                             ("random A, dA", lambda: GraphIsoConvTD([12, 12]), td_case)):
        src, x, A, _, _ = case(name, dev)
        x, A = x.to(dev), A.to(dev).contiguous()
        src(x, A, True)                                # the moving statistics leave their start
        dst = make()
        dst.load_state_dict(src.state_dict())          # dst has never been called: built from the first kernel's shape
        assert set(dst.state_dict()) == set(src.state_dict())
        assert torch.equal(dst(x, A, False)[0], src(x, A, False)[0])
        assert torch.equal(dst(x, A, True)[0], src(x, A, True)[0])


@pytest.mark.parametrize("which", ["iso", "td"])
def test_inference_uses_the_moving_statistics_and_leaves_them(dev, which):
    layer, x, A, dout, _ = iso_case("two layers, dA", dev) if which == "iso" else td_case("random A, dA", dev)
    xd, Ad = x.to(dev), A.to(dev).contiguous()
    for _ in range(2):
        layer(xd, Ad, True)
    before = {k: v.clone() for k, v in layer.state_dict().items()}
    out, _ = layer(xd, Ad, False)
    ref = reference(layer, x, A, dout, False, training=False)[0]
    print("%s inference: out %.2e" % (which, rel_err(out, ref)))
    assert rel_err(out, ref) < BAR
    assert all(torch.equal(v, before[k]) for k, v in layer.state_dict().items())
    layer.eval()                                       # training=None follows the module's mode
    assert torch.equal(layer(xd, Ad)[0], out)
    layer.train()
    assert torch.equal(layer(xd, Ad)[0], layer(xd, Ad, True)[0])
    y, _ = layer(xd.clone().requires_grad_(True), Ad, False)
    with pytest.raises(RuntimeError, match="training=False"):
        y.sum().backward()


@pytest.mark.parametrize("which", ["iso", "td"])
def test_two_calls_then_both_backwards(dev, which):
    """the layer keeps everything backward needs in ctx: two forward calls of one instance, then both backwards, give the gradients of
    the two calls run one after the other"""
    layer, x, A, dout, _ = iso_case("two layers, dA", dev) if which == "iso" else td_case("random A, dA", dev)
    x1, x2 = x.to(dev), (0.5 * x + 0.1).to(dev)
    Ad, d = A.to(dev).contiguous(), dout.to(dev)
    params = list(layer.parameters())

    def grads(out, xg, Ag):
        return torch.autograd.grad(out, [xg, Ag] + params, d)
    separate = []
    for xs in (x1, x2):
        xg, Ag = xs.clone().requires_grad_(True), Ad.clone().requires_grad_(True)
        separate.append(grads(layer(xg, Ag, True)[0], xg, Ag))
    leaves = [(xs.clone().requires_grad_(True), Ad.clone().requires_grad_(True)) for xs in (x1, x2)]
    outs = [layer(xg, Ag, True)[0] for xg, Ag in leaves]
    together = [grads(o, xg, Ag) for o, (xg, Ag) in zip(outs, leaves)]
    for a, b in zip(separate, together):
        assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_bad_arguments_raise_value_error_before_any_launch(dev):
    x3, A3 = _randn(3, 16, 25, seed=21).to(dev), _randn(3, 25, 25, seed=22).to(dev)
    x4, A4 = _randn(2, 16, 4, 25, seed=23).to(dev), _randn(2, 25, 25, seed=24).to(dev)
    for cls in (GraphIsoConv, GraphIsoConvTD):
        with pytest.raises(ValueError, match="tanh"):
            cls([8], activation="tanh")
        with pytest.raises(ValueError, match="ncw,nvw->ncv"):
            cls([8], einsum="ncw,nvw->ncv")
        for filters in ([], 8, (8, 8), None):
            with pytest.raises(ValueError, match="filters"):
                cls(filters)
    with pytest.raises(ValueError, match="return_logits"):
        GraphIsoConvTD([8], return_logits=True)
    with pytest.raises(ValueError, match="kernel_size"):
        GraphIsoConvTD([8], kernel_size=9)
    iso, td = GraphIsoConv([8]), GraphIsoConvTD([8])
    for bad in (lambda: iso(x3.transpose(1, 2), A3, True), lambda: iso(x3.cpu(), A3, True), lambda: iso(x3, A3.cpu(), True),
                lambda: iso(x3.double(), A3, True), lambda: iso(x3, A3[:2], True),
                lambda: iso(torch.zeros(1, 2, 513, device=dev), torch.zeros(1, 513, 513, device=dev), True),      # V > 512
                lambda: td(x4.permute(0, 1, 3, 2), A4, True), lambda: td(x4.cpu(), A4, True), lambda: td(x4, A4[:1], True),
                lambda: td(torch.zeros(1, 2, 2, 33, device=dev), torch.zeros(2, 33, 33, device=dev), True)):      # V > 32
        with pytest.raises(ValueError):
            bad()
    assert iso.epsilon is None and td.epsilon is None          # nothing was built, nothing launched
    with pytest.raises(ValueError, match="N \\* V"):
        iso(torch.zeros(1 << 22, 1, 1, device=dev), torch.zeros(1 << 22, 1, 1, device=dev), True)      # N V = 2^22
    assert iso.epsilon is None
    iso(x3, A3, True)
    with pytest.raises(ValueError, match="16 input channels"):
        iso(x3[:, :8].contiguous(), A3, True)
