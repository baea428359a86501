"""GPU: TemporalAttention (csrc/tattn.hip through the C ABI, sar_amd.ops, and the module models.stgcn.TemporalAttention) against the
float64 restatement tests/tattn_reference.py over the cases of tests/tattn_cases.py.

Each of the five kernels runs on its own, its inputs the float64 reference's intermediates rounded to float32, and is judged against
float64; then the whole layer runs through ops and through the module (out, a, dx and every dkernel / dbias).

Tolerance (the rule of tests/test_gpu_pgpool.py): norm-wise relative error (tests/util.rel_err) below TOL = 2e-5; a quantity that
misses TOL is judged against 8x the distance of the float32 run of the SAME restatement (CPU) from float64 -- the band matters for a
last-layer bias gradient whose terms cancel (4e-5 in the float32 restatement at (2, 16, 300, 25)).  Both numbers are printed.
tests/test_tattn_reference.py asserts that no case has a hidden pre-activation within 1e-5 RMS of zero.

Worst errors observed on MI355X per quantity: profiles/tattn.txt."""
import pytest
import torch

import tattn_cases as K
from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
RELU, SIGMOID = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def judge(name, got, ref64, ref32):
    e, band = rel_err(got, ref64), rel_err(ref32, ref64)
    print("%-12s engine %.3e, float32 restatement %.3e from float64" % (name, e, band))
    return None if (e < TOL or e <= 8 * band) else (e, band)


def assert_all(pairs):
    bad = {k: v for k, v in pairs.items() if v is not None}
    assert not bad, "(engine error, float32 band) beyond TOL and 8x the band: %s" % bad


def f32(t, dev):
    return t.to(torch.float32).to(dev).contiguous()


def kernels(dev, case):
    """the five entry points one at a time on the float64 reference's intermediates rounded to float32 -> dict of their results"""
    from sar_amd import _lib as L
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, T, V, hidden, _ = case
    (x, dout, params), r64, _ = K.reference(case)
    lib, st, n, u = L.load(), stream_ptr(), N * T, params[0].shape[1]
    xd, dd, k1, b1 = f32(x, dev), f32(dout, dev), f32(params[0], dev), f32(params[1], dev)
    a, dz1 = f32(r64["a"], dev), f32(r64["dz1"], dev)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    sn, sc = C * T * V, T * V
    h1, out, dzL, dx = new(u, n), new(N, C, T, V), new(n), new(N, C, T, V)
    check(lib.sar_tattn_score_f32(ptr(xd), sn, sc, ptr(k1), ptr(b1), N, C, T, V, u, SIGMOID if not hidden else RELU, ptr(h1), n, st), "score")
    check(lib.sar_tattn_scale_f32(ptr(xd), sn, sc, ptr(a), N, C, T, V, ptr(out), sn, sc, st), "scale")
    check(lib.sar_tattn_dscore_f32(ptr(xd), sn, sc, ptr(dd), sn, sc, ptr(a), N, C, T, V, ptr(dzL), st), "dscore")
    nslab, size = lib.sar_tattn_wgrad_slabs(N, C, T, V), V * C * u + u
    slab, flat = new(nslab, size), new(size)
    check(lib.sar_tattn_wgrad_f32(ptr(xd), sn, sc, ptr(dz1), n, N, C, T, V, u, ptr(slab), nslab, st), "wgrad")
    check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(flat), st), "slab_reduce")
    check(lib.sar_tattn_dx_f32(ptr(dd), sn, sc, ptr(a), ptr(k1), ptr(dz1), n, N, C, T, V, u, ptr(dx), sn, sc, st), "dx")
    torch.cuda.synchronize()
    return dict(h1=h1, out=out, dzL=dzL, dkernel1=flat[:V * C * u].view(V * C, u), dbias1=flat[V * C * u:], dx=dx)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_each_kernel_matches_the_float64_restatement(dev, case):
    _, r64, r32 = K.reference(case)
    got = kernels(dev, case)
    want = lambda r: dict(h1=r["h1"], out=r["out"], dzL=r["dzL"], dkernel1=r["grads"][0], dbias1=r["grads"][1], dx=r["dx"])
    w64, w32 = want(r64), want(r32)
    assert_all({k: judge(k, got[k], w64[k], w32[k]) for k in w64})


def run_ops(dev, case, need_dx=True):
    from sar_amd import ops
    (x, dout, params), _, _ = K.reference(case)
    xd, dd, pd = f32(x, dev), f32(dout, dev), [f32(p, dev) for p in params]
    out, saved = ops.tattn_forward(xd, pd)
    dx, grads = ops.tattn_backward(xd, saved, pd, dd, need_dx=need_dx)
    torch.cuda.synchronize()
    return dict(out=out, a=saved[0], dx=dx, grads=grads)


def judge_layer(got, r64, r32):
    pairs = {k: judge(k, got[k], r64[k], r32[k]) for k in ("out", "a", "dx") if got[k] is not None}
    for i, g in enumerate(got["grads"]):
        name = "%s_%d" % ("dbias" if i % 2 else "dkernel", i // 2 + 1)
        pairs[name] = judge(name, g.reshape(r64["grads"][i].shape), r64["grads"][i], r32["grads"][i])
    assert_all(pairs)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_layer_through_ops_matches_the_float64_restatement(dev, case):
    _, r64, r32 = K.reference(case)
    judge_layer(run_ops(dev, case), r64, r32)


def make_module(dev, case):
    from models.stgcn import TemporalAttention
    (x, dout, params), _, _ = K.reference(case)
    m = TemporalAttention(list(case[4]))
    m.load_state_dict({"mlp.%d.%s" % (i // 2, "bias" if i % 2 else "kernel"): f32(p, dev) for i, p in enumerate(params)})
    return m, f32(x, dev), f32(dout, dev)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_module_matches_the_float64_restatement(dev, case):
    N, C, T, V = case[:4]
    _, r64, r32 = K.reference(case)
    m, xd, dd = make_module(dev, case)
    xd.requires_grad_()
    out = m(xd, True)
    out.backward(dd)
    torch.cuda.synchronize()
    assert tuple(m.last_attention.shape) == (N, T) and not m.last_attention.requires_grad
    got = dict(out=out.detach(), a=m.last_attention.reshape(-1), dx=xd.grad, grads=[p.grad for layer in m.mlp for p in (layer.kernel, layer.bias)])
    judge_layer(got, r64, r32)


@pytest.mark.parametrize("case", [K.LISTED[1], K.LISTED[2], K.LISTED[5], K.EDGES[0]], ids=K.case_id)
def test_two_runs_are_bitwise_equal(dev, case):
    a, b = run_ops(dev, case), run_ops(dev, case)
    for k in ("out", "a", "dx"):
        assert torch.equal(a[k], b[k]), k
    for i, (g, h) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(g, h), "grads[%d]" % i


def test_need_dx_false_returns_no_dx_and_the_same_gradients(dev):
    a, b = run_ops(dev, K.LISTED[4]), run_ops(dev, K.LISTED[4], need_dx=False)
    assert b["dx"] is None and all(torch.equal(g, h) for g, h in zip(a["grads"], b["grads"]))


def test_a_sample_does_not_depend_on_the_rest_of_the_batch(dev):
    """(32, 64, 75, 25), num_hidden [64]: every 8-sample slice of out and dx is bitwise the N = 8 run on that slice (parameter gradients
    are batch sums and are not compared)"""
    from sar_amd import ops
    N, C, T, V = 32, 64, 75, 25
    gen = torch.Generator().manual_seed(3)
    x, dout = (torch.randn(N, C, T, V, generator=gen).to(dev) for _ in range(2))
    params = [f32(p, dev) for p in K.make_params(C, V, (64,), gen)]
    out, saved = ops.tattn_forward(x, params)
    dx, _ = ops.tattn_backward(x, saved, params, dout)
    for n0 in range(0, N, 8):
        xs, ds = x[n0:n0 + 8], dout[n0:n0 + 8]
        o8, s8 = ops.tattn_forward(xs, params)
        d8, _ = ops.tattn_backward(xs, s8, params, ds)
        assert torch.equal(o8, out[n0:n0 + 8]), "out, samples %d.." % n0
        assert torch.equal(d8, dx[n0:n0 + 8]), "dx, samples %d.." % n0


@pytest.mark.parametrize("case", [K.LISTED[0], K.LISTED[4], K.EDGES[0]], ids=K.case_id)
def test_cn_views_give_the_nchw_bits(dev, case):
    """x, out, dout and dx as views of CN matrices [C][N T V + 3] (s_n = T V, s_c = ld): bitwise what the NCHW tensors give"""
    from sar_amd import ops
    N, C, T, V = case[:4]
    (x, dout, params), _, _ = K.reference(case)
    pd = [f32(p, dev) for p in params]
    want = run_ops(dev, case)
    ld = N * T * V + 3

    def cn(t=None):
        m = torch.full((C, ld), float("nan"), dtype=torch.float32, device=dev)
        view = m[:, :N * T * V].view(C, N, T, V).permute(1, 0, 2, 3)
        if t is not None:
            view.copy_(t.to(torch.float32))
        return view
    xv, dv, ov, gv = cn(x), cn(dout), cn(), cn()
    out, saved = ops.tattn_forward(xv, pd, out=ov)
    dx, grads = ops.tattn_backward(xv, saved, pd, dv, dx=gv)
    assert out is ov and dx is gv
    assert torch.equal(out, want["out"]) and torch.equal(dx, want["dx"]) and torch.equal(saved[0], want["a"])
    assert all(torch.equal(g, h) for g, h in zip(grads, want["grads"]))


def test_attention_in_front_of_the_model_trains_under_one_optimizer(dev):
    """TemporalAttention -> models.stgcn.Model: the engine hands d loss / d clip back, every parameter of the gate
    gets a finite, non-zero gradient, and one optimizer step moves both"""
    from models.stgcn import Model, TemporalAttention
    from oracle import stgcn as O
    N, C, T, V, M = 2, 3, 10, 25, 2
    torch.manual_seed(0)
    gate = TemporalAttention([8])
    model = Model(num_classes=10, device=dev, seed=2, blocks=[(64, 1, False), (64, 1, True)])
    x, y = O.synthetic_batch(N, seed=5, T=T, num_classes=10)
    x, y = x.to(dev), y.to(dev)
    gate(x.reshape(N, C, T, V * M))                                      # the first call builds the gate's parameters
    opt = torch.optim.SGD(list(gate.parameters()) + list(model.parameters()), lr=0.01, momentum=0.9, nesterov=True)
    before = [p.detach().clone() for p in gate.parameters()]
    clip = gate(x.reshape(N, C, T, V * M), True).view(N, C, T, V, M)
    loss = torch.nn.functional.cross_entropy(model(clip, True), y)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert len(before) == 4 and tuple(gate.last_attention.shape) == (N, T)
    for (name, p), old in zip(gate.named_parameters(), before):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max().item() > 0, name
        assert not torch.equal(p.detach(), old), name


def test_module_creates_its_parameters_lazily_with_the_glorot_limit(dev):
    from models.stgcn import TemporalAttention
    N, C, T, V = 2, 64, 9, 25
    m = TemporalAttention([48, 16])
    assert list(m.parameters()) == []
    torch.manual_seed(0)
    out = m(torch.randn(N, C, T, V, device=dev), True)
    assert tuple(out.shape) == (N, C, T, V)
    assert [n for n, _ in m.named_parameters()] == ["mlp.%d.%s" % (i, k) for i in range(3) for k in ("kernel", "bias")]
    for layer, (fan_in, units) in zip(m.mlp, ((V * C, 48), (48, 16), (16, 1))):
        limit = (6.0 / (fan_in + units)) ** 0.5
        k = layer.kernel.detach()
        assert tuple(k.shape) == (fan_in, units) and k.is_cuda and float(k.abs().max()) <= limit
        if k.numel() >= 512:
            assert float(k.abs().max()) > 0.9 * limit and abs(float(k.std()) - limit / 3 ** 0.5) < 0.1 * limit
        assert tuple(layer.bias.shape) == (units,) and not bool(layer.bias.detach().any())
    with pytest.raises(ValueError, match="input features"):
        m(torch.randn(N, C + 1, T, V, device=dev), True)


def test_module_round_trips_a_state_dict(dev):
    from models.stgcn import TemporalAttention
    case = K.LISTED[0]
    m, xd, _ = make_module(dev, case)
    want = m(xd, False)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    assert sorted(state) == ["mlp.0.bias", "mlp.0.kernel", "mlp.1.bias", "mlp.1.kernel"]
    m2 = TemporalAttention(list(case[4]))
    m2.load_state_dict(state)
    assert torch.equal(m2(xd, False), want) and torch.equal(m2.last_attention, m.last_attention)


def test_module_gives_the_gradient_of_a_loss_on_a_slice_of_out(dev):
    """the loss reads out[:, :, 1::2]: dout arrives as zeros outside the slice"""
    import tattn_reference as R
    case = K.LISTED[0]
    (x, _, params), _, _ = K.reference(case)
    m, xd, _ = make_module(dev, case)
    xd.requires_grad_()
    w = torch.randn(x[:, :, 1::2].shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (m(xd, True)[:, :, 1::2] * f32(w, dev)).sum().backward()
    dout = torch.zeros_like(x)
    dout[:, :, 1::2] = w
    runs = []
    for dt in (torch.float64, torch.float32):
        _, ctx = R.forward(x.to(dt), [p.to(dt) for p in params])
        dx, grads, _ = R.backward(ctx, dout.to(dt))
        runs.append(dict(dx=dx, grads=grads))
    got = dict(out=None, a=None, dx=xd.grad, grads=[p.grad for layer in m.mlp for p in (layer.kernel, layer.bias)])
    pairs = {"dx": judge("dx", got["dx"], runs[0]["dx"], runs[1]["dx"])}
    for i, g in enumerate(got["grads"]):
        pairs["grads[%d]" % i] = judge("grads[%d]" % i, g.reshape(runs[0]["grads"][i].shape), runs[0]["grads"][i], runs[1]["grads"][i])
    assert_all(pairs)


def test_module_saves_nothing_under_no_grad(dev):
    m, xd, _ = make_module(dev, K.LISTED[0])
    with torch.no_grad():
        out = m(xd, True)
    assert out.grad_fn is None and not out.requires_grad
    for p in m.parameters():
        p.requires_grad_(False)
    out = m(xd, True)                                        # nothing requires a gradient
    assert out.grad_fn is None and not out.requires_grad
    for p in m.parameters():
        p.requires_grad_(True)
    seen = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t) or t, lambda t: t):
        with torch.no_grad():
            m(xd, True)
        assert seen == []
        m(xd, True)
    assert len(seen) == 1 + 2 + 4                            # x, (a, h_1), two kernels and two biases


def test_module_rejects_what_it_is_not_built_for(dev):
    from models.stgcn import TemporalAttention
    m = TemporalAttention([6])
    x = torch.randn(2, 4, 6, 5, device=dev)
    for bad in (x.double(), x[:, :, ::2], x.cpu(), x[0], torch.randn(2, 4, 6, 65, device=dev), x[:0]):
        with pytest.raises(ValueError):
            m(bad, True)
    assert list(m.parameters()) == [] and m.last_attention is None, "a rejected call built or launched something"
