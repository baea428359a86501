"""GPU: ProjectionGraphPool (csrc/pgpool.hip through sar_amd.ops, and the module models/stpgcnp.py) against the float64 restatement
tests/pgpool_reference.py.

Tolerance (the rule of tests/test_gpu_stpgcn.py): norm-wise relative error (tests/util.rel_err) below TOL = 1e-4; a quantity that
misses TOL is judged against 8x the distance of the float32 run of the SAME restatement (CPU, difference-form distance) from
float64 -- at the reference's initialisation the logits are ~ -250 and differ by ~ 0.5 between vertices, so float32 itself is
1.6e-5 (q) to 4e-5 (dx) away and a fixed 1e-4 cannot judge the layer.  Both numbers are printed.  Every case first asserts, on the
float64 reference alone: min qs >= 1e-3, min d > 1e-9 (the clamp never binds), min sum_j zp^2 >= 1e-6.

Worst errors observed on MI355X per quantity: profiles/pgpool.txt."""
import functools

import pytest
import torch

import pgpool_reference as R
from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(3, 40, 37, 24),        # nothing a multiple of anything
          (2, 64, 130, 33),       # odd J, P just over a 128 tile
          (2, 256, 75, 512),      # the first pool at 3 frames
          (2, 256, 512, 256)]     # the second pool
REGIMES = ["spread", "init"]
SEED = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(regime, shape):
    """(inputs, float64 results, float32 results) of one case, computed once and shared; results = dict of q, zn, A_out, dx, dcenters,
    dvariance"""
    B, C, P, J = shape
    x, cen, var = R.make_case(regime, B, C, P, J, SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    dz = torch.randn(B, C, J, generator=g, dtype=torch.float64)
    dA = torch.randn(B, J, J, generator=g, dtype=torch.float64)          # not symmetric
    out = []
    for dt in (torch.float64, torch.float32):
        zn, A, ctx = R.pool_forward(x.to(dt), cen.to(dt), var.to(dt))
        if dt == torch.float64:
            qs_min, d_min, n2_min = R.preconditions(ctx)
            assert qs_min >= 1e-3 and d_min > 1e-9 and n2_min >= 1e-6, (regime, shape, qs_min, d_min, n2_min)
        dx, dcen, dvar = R.pool_backward(ctx, dz.to(dt), dA.to(dt))
        out.append(dict(q=ctx["q"], zn=zn, A_out=A, dx=dx, dcenters=dcen, dvariance=dvar))
    return (x, cen, var, dz, dA), out[0], out[1]


def judge(name, got, ref64, ref32):
    e, band = rel_err(got, ref64), rel_err(ref32, ref64)
    print("%-10s engine %.3e, float32 restatement %.3e from float64" % (name, e, band))
    return None if (e < TOL or e <= 8 * band) else (e, band)


def run_ops(dev, shape, x, cen, var, dz, dA):
    """the layer through sar_amd.ops on CN operands -> dict of the compared quantities in the reference's layouts"""
    from sar_amd import ops
    B, C, P, J = shape
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    X = f(x.permute(1, 0, 2).reshape(C, B * P))
    cen_d, var_d = f(cen), f(var)
    zn, A, saved = ops.pgpool_forward(X, B, P, cen_d, var_d)
    dX, dcen, dvar = torch.empty_like(X), torch.empty_like(cen_d), torch.empty_like(var_d)
    ops.pgpool_backward(X, B, P, cen_d, zn, saved, f(dz), f(dA), dX, dcen, dvar)
    torch.cuda.synchronize()
    return dict(q=saved[0].reshape(J, B, P).permute(1, 2, 0), zn=zn, A_out=A, dx=dX.reshape(C, B, P).permute(1, 0, 2), dcenters=dcen,
                dvariance=dvar)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_matches_the_float64_restatement(dev, shape, regime):
    inputs, ref64, ref32 = reference(regime, shape)
    got = run_ops(dev, shape, *inputs)
    bad = {k: judge(k, got[k], ref64[k], ref32[k]) for k in ref64}
    bad = {k: v for k, v in bad.items() if v is not None}
    assert not bad, "(engine error, float32 band) beyond TOL and 8x the band: %s" % bad


@pytest.mark.parametrize("shape,regime", [((2, 70, 20, 256), "spread"), ((2, 70, 20, 256), "init"),      # one vertex per lane in assign ...
                                          ((2, 70, 20, 257), "spread"), ((2, 70, 20, 257), "init"),      # ... and two; C over a 64-channel chunk
                                          ((1, 512, 9, 512), "init"),                                    # the largest C and J
                                          ((2, 5, 1, 3), "spread"), ((2, 5, 1, 3), "init")],             # one column per sample
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_sizes_at_which_the_kernels_take_another_path(dev, shape, regime):
    inputs, ref64, ref32 = reference(regime, shape)
    got = run_ops(dev, shape, *inputs)
    bad = {k: judge(k, got[k], ref64[k], ref32[k]) for k in ref64}
    bad = {k: v for k, v in bad.items() if v is not None}
    assert not bad, "(engine error, float32 band) beyond TOL and 8x the band: %s" % bad


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_are_bitwise_equal(dev, shape):
    inputs, _, _ = reference("init", shape)
    a, b = run_ops(dev, shape, *inputs), run_ops(dev, shape, *inputs)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_sample_does_not_depend_on_the_rest_of_the_batch(dev):
    """(128, 256, 950, 512), the benchmark batch of the first pool: every 8-sample slice of zn, A_out and dx is bitwise the B = 8
    run on that slice (operands of the slices are row-strided views of the batch's)"""
    from sar_amd import ops
    B, C, P, J, Bs = 128, 256, 950, 512, 8
    g = torch.Generator(device=dev).manual_seed(3)
    X = torch.relu(torch.randn(C, B * P, generator=g, device=dev))
    lim = R.glorot_limit(C, J)
    cen = (torch.rand(1, C, 1, J, generator=g, device=dev) * 2 - 1) * lim
    var = (torch.rand(1, C, 1, J, generator=g, device=dev) * 2 - 1) * lim
    dz = torch.randn(B, C, J, generator=g, device=dev)
    dA = torch.randn(B, J, J, generator=g, device=dev)

    def run(Xv, n, dzv, dAv):
        zn, A, saved = ops.pgpool_forward(Xv, n, P, cen, var)
        dX, dcen, dvar = torch.empty((C, n * P), device=dev), torch.empty_like(cen), torch.empty_like(var)
        ops.pgpool_backward(Xv, n, P, cen, zn, saved, dzv, dAv, dX, dcen, dvar)
        return zn, A, dX

    zn, A, dX = run(X, B, dz, dA)
    assert bool(torch.isfinite(zn).all()) and bool(torch.isfinite(A).all()) and bool(torch.isfinite(dX).all())
    for i in range(0, B, Bs):
        cols = slice(i * P, (i + Bs) * P)
        zn_s, A_s, dX_s = run(X[:, cols], Bs, dz[i:i + Bs], dA[i:i + Bs])
        assert torch.equal(zn_s, zn[i:i + Bs]), "zn, samples %d.." % i
        assert torch.equal(A_s, A[i:i + Bs]), "A_out, samples %d.." % i
        assert torch.equal(dX_s, dX[:, cols]), "dx, samples %d.." % i


# ---- the module
def _module_inputs(dev, shape=(3, 40, 37, 24), regime="spread"):
    (x, cen, var, dz, dA), ref64, ref32 = reference(regime, shape)
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    return f(x), f(cen), f(var), f(dz), f(dA), ref64, ref32


def test_module_creates_its_parameters_lazily_and_trains(dev):
    from models.stpgcnp import ProjectionGraphPool
    x, cen, var, dz, dA, ref64, ref32 = _module_inputs(dev)
    layer = ProjectionGraphPool(24)
    assert layer.centers is None and layer.variance is None and not list(layer.parameters())
    torch.manual_seed(7)
    layer(x, None)
    assert tuple(layer.centers.shape) == (1, 40, 1, 24) == tuple(layer.variance.shape) and layer.centers.is_cuda
    limit = R.glorot_limit(40, 24)
    for p in (layer.centers, layer.variance):
        assert 0.8 * limit < p.abs().max().item() <= limit and abs(p.mean().item()) < 0.2 * limit
    assert not torch.equal(layer.centers, layer.variance)
    with torch.no_grad():
        layer.centers.copy_(cen), layer.variance.copy_(var)
    xr = x.clone().requires_grad_(True)
    z, A = layer(xr, torch.zeros(3, 5, 5, device=dev), training=True)       # (the incoming A is ignored)
    torch.autograd.backward([z, A], [dz, dA])
    got = dict(zn=z, A_out=A, dx=xr.grad, dcenters=layer.centers.grad, dvariance=layer.variance.grad)
    assert not {k: v for k, v in ((k, judge(k, got[k], ref64[k], ref32[k])) for k in got) if v is not None}
    with pytest.raises(ValueError):
        layer(torch.zeros(3, 41, 37, device=dev))                            # built for 40 channels


def test_module_gradient_of_one_output_alone(dev):
    """autograd hands None for the output that was not used: it counts as zero"""
    from models.stpgcnp import ProjectionGraphPool
    x, cen, var, dz, dA, _, _ = _module_inputs(dev)
    layer = ProjectionGraphPool(24)
    layer.load_state_dict({"centers": cen, "variance": var})
    grads = []
    for use_z, use_A in ((True, False), (False, True), (True, True)):
        xr = x.clone().requires_grad_(True)
        z, A = layer(xr, None)
        loss = (z * dz).sum() * use_z + (A * dA).sum() * use_A
        grads.append(torch.autograd.grad(loss, [xr, layer.centers, layer.variance]))
    for gz, gA, both in zip(*grads):
        assert rel_err(gz + gA, both) < 1e-5


def test_module_state_dict_round_trip(dev):
    from models.stpgcnp import ProjectionGraphPool
    x = _module_inputs(dev)[0]
    a = ProjectionGraphPool(24)
    za, Aa = a(x, None)
    sd = a.state_dict()
    assert set(sd) == {"centers", "variance"}
    b = ProjectionGraphPool(24)
    b.load_state_dict({k: v.cpu() for k, v in sd.items()})                   # builds the parameters from the state dict
    assert b.centers.is_cuda and torch.equal(b.centers, a.centers) and torch.equal(b.variance, a.variance)
    zb, Ab = b(x, None)
    assert torch.equal(za, zb) and torch.equal(Aa, Ab)


def test_module_flattens_trailing_dimensions(dev):
    from models.stpgcnp import ProjectionGraphPool
    g = torch.Generator().manual_seed(5)
    x4 = (0.3 * torch.relu(torch.randn(2, 16, 6, 5, generator=g))).to(dev)
    layer = ProjectionGraphPool(7)
    z4, A4 = layer(x4, None)
    z3, A3 = layer(x4.reshape(2, 16, 30), None)
    assert tuple(z4.shape) == (2, 16, 7) and tuple(A4.shape) == (2, 7, 7)
    assert torch.equal(z4, z3) and torch.equal(A4, A3)


def test_module_rejects_what_it_is_not_built_for(dev):
    from models.stpgcnp import ProjectionGraphPool
    with pytest.raises(ValueError):
        ProjectionGraphPool(513)
    layer = ProjectionGraphPool(8)
    x = torch.rand(2, 16, 30, device=dev)
    for bad in (x.cpu(), x.double(), x.transpose(1, 2), torch.rand(2, 513, 4, device=dev)):
        with pytest.raises(ValueError):
            layer(bad, None)
    assert layer.centers is None                                             # nothing was built, nothing launched


def test_pool_graphconv_chain_under_autograd(dev):
    """ProjectionGraphPool(24) -> GraphConv(32) -> ProjectionGraphPool(12) -> GraphConv(48) at C = 32, P = 50 against the float64
    composition (models/stpgcnp.py:141-144 and 170-171 of the reference, at test sizes)"""
    from models.gcn import GraphConv
    from models.stpgcnp import ProjectionGraphPool
    B, C, P, verts, filt = 2, 32, 50, (24, 12), (32, 48)
    g = torch.Generator().manual_seed(11)
    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)
    x = 0.3 * torch.relu(rn(B, C, P))
    params = {"p0.centers": 0.05 * rn(1, C, 1, verts[0]), "p0.variance": 0.5 * rn(1, C, 1, verts[0]),
              # (a small first GraphConv: its output is the second pool's x, which has to stay O(0.3) for every vertex to keep mass)
              "g0.kernel": 0.002 * rn(1, C, filt[0]), "g0.bias": 0.003 * rn(filt[0]),
              "p1.centers": 0.05 * rn(1, filt[0], 1, verts[1]), "p1.variance": 0.5 * rn(1, filt[0], 1, verts[1]),
              "g1.kernel": 0.2 * rn(1, filt[0], filt[1]), "g1.bias": 0.1 * rn(filt[1])}
    dout = rn(B, filt[1], verts[1])

    def oracle(dt):
        leaves = {k: v.to(dt).clone().requires_grad_(True) for k, v in params.items()}
        xr = x.to(dt).clone().requires_grad_(True)
        h = xr
        for i in range(2):
            if dt == torch.float64:                                          # the preconditions, for both pools
                qs_min, d_min, n2_min = R.preconditions(R.pool_forward(h.detach(), params["p%d.centers" % i], params["p%d.variance" % i])[2])
                assert qs_min >= 1e-3 and d_min > 1e-9 and n2_min >= 1e-6, (i, qs_min, d_min, n2_min)
            h, A = R.Pool.apply(h, leaves["p%d.centers" % i], leaves["p%d.variance" % i])
            hg = torch.einsum("cf,ncv->nfv", leaves["g%d.kernel" % i][0], h) + leaves["g%d.bias" % i][None, :, None]
            h = torch.einsum("ncv,nvw->ncw", hg, A)
        grads = torch.autograd.grad((h * dout.to(dt)).sum(), [xr] + list(leaves.values()))
        res = {"out": h.detach(), "dx": grads[0]}
        res.update({"d" + k: v for k, v in zip(leaves, grads[1:])})
        return res

    ref64, ref32 = oracle(torch.float64), oracle(torch.float32)
    layers = [ProjectionGraphPool(verts[0]), GraphConv(filt[0]), ProjectionGraphPool(verts[1]), GraphConv(filt[1])]
    f = lambda t: t.to(torch.float32).to(dev).contiguous()
    layers[0].load_state_dict({"centers": f(params["p0.centers"]), "variance": f(params["p0.variance"])})
    layers[1].load_state_dict({"kernel": f(params["g0.kernel"]), "bias": f(params["g0.bias"])})
    layers[2].load_state_dict({"centers": f(params["p1.centers"]), "variance": f(params["p1.variance"])})
    layers[3].load_state_dict({"kernel": f(params["g1.kernel"]), "bias": f(params["g1.bias"])})
    xr = f(x).requires_grad_(True)
    h, A = xr, None
    for l in layers:
        h, A = l(h, A, training=True)
    (h * f(dout)).sum().backward()
    got = {"out": h, "dx": xr.grad,
           "dp0.centers": layers[0].centers.grad, "dp0.variance": layers[0].variance.grad,
           "dg0.kernel": layers[1].kernel.grad, "dg0.bias": layers[1].bias.grad,
           "dp1.centers": layers[2].centers.grad, "dp1.variance": layers[2].variance.grad,
           "dg1.kernel": layers[3].kernel.grad, "dg1.bias": layers[3].bias.grad}
    bad = {k: v for k, v in ((k, judge(k, got[k], ref64[k], ref32[k])) for k in got) if v is not None}
    assert not bad, bad
