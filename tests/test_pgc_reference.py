"""The float64 restatement of ProjectionGraphConv (tests/pgc_reference.py) pinned before the GPU tests rely on it: an independent
numpy forward, central finite differences of its hand-written backward pass, and the engine's initialisation of centers / variance
(Keras glorot_uniform for the (1, 64, 1, 32) weights: U(-0.0533, 0.0533))."""
import math

import numpy as np
import pytest
import torch

import pgc_reference as R

B, C, T, V, J = 2, 8, 5, 25, 4


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, C, T, V, generator=g, dtype=torch.float64))
    cen = 0.5 * torch.randn(1, C, 1, J, generator=g, dtype=torch.float64)
    var = 0.5 * torch.randn(1, C, 1, J, generator=g, dtype=torch.float64)
    W = 0.3 * torch.randn(1, C, C, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    return x, cen, var, W, b


def _numpy_forward(x, cen, var, W, b):
    """the reference's call() line by line (models/stpgcn.py:23-47), z materialised"""
    x, cen, var, W, b = (t.numpy() for t in (x, cen, var, W, b))
    N, Cc, Tt, Vv = x.shape
    z = (x.reshape(N, Cc, -1, 1) - cen) / (1 / (1 + np.exp(-var)))           # (N, C, P, J)
    q = np.maximum(np.sum(z ** 2, axis=1), 1e-12) * (-1 / 2)                  # (N, P, J)
    q = np.exp(q - q.max(-1, keepdims=True))
    q /= q.sum(-1, keepdims=True)
    zz = np.sum(q[:, None] * z, axis=-2) / np.sum(q, axis=-2, keepdims=True)  # (N, C, J)
    zz = zz / np.sqrt(np.maximum(np.sum(zz ** 2, axis=-1, keepdims=True), 1e-12))
    A = np.matmul(np.transpose(zz, (0, 2, 1)), zz)
    g = np.einsum("cf,ncv->nfv", W[0], zz) + b[None, :, None]
    g = np.einsum("ncv,nvw->ncw", g, A)
    xp = np.transpose(np.matmul(q, np.transpose(g, (0, 2, 1))), (0, 2, 1)).reshape(N, -1, Tt, Vv)
    return x + xp, q, zz, A


def test_forward_matches_an_independent_numpy_restatement():
    args = _inputs()
    out, ctx = R.pgc_forward(*args)
    ref, q, zn, A = _numpy_forward(*args)
    for got, want in ((out, ref), (ctx["q"], q), (ctx["zn"], zn), (ctx["A"], A)):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_backward_matches_central_finite_differences():
    args = list(_inputs(1))
    g = torch.Generator().manual_seed(2)
    dout = torch.randn(B, C, T, V, generator=g, dtype=torch.float64)
    _, ctx = R.pgc_forward(*args)
    grads = R.pgc_backward(ctx, dout)

    def f(a):
        return (R.pgc_forward(*a)[0] * dout).sum().item()

    h = 1e-6
    rng = np.random.default_rng(3)
    for i, (a, ga) in enumerate(zip(args, grads)):
        flat = a.view(-1)
        idx = rng.choice(flat.numel(), size=min(24, flat.numel()), replace=False)
        for k in idx:
            old = flat[k].item()
            flat[k] = old + h
            fp = f(args)
            flat[k] = old - h
            fm = f(args)
            flat[k] = old
            fd = (fp - fm) / (2 * h)
            an = ga.reshape(-1)[k].item()
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)), (i, int(k), fd, an)


def test_autograd_function_matches_the_plain_backward():
    args = [t.clone().requires_grad_(True) for t in _inputs(4)]
    out = R.PGC.apply(*args)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    out.backward(dout)
    _, ctx = R.pgc_forward(*[t.detach() for t in args])
    for a, want in zip(args, R.pgc_backward(ctx, dout)):
        assert torch.equal(a.grad, want)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_centers_and_variance_init_is_glorot_uniform(seed):
    from sar_amd.stpgcn import glorot_uniform
    limit = math.sqrt(6.0 / (64 + 32 * 64))
    assert abs(limit - 0.0533) < 1e-4
    w = glorot_uniform((1, 64, 1, 32), torch.Generator().manual_seed(seed))
    assert w.shape == (1, 64, 1, 32)
    assert w.abs().max().item() <= limit
    assert abs(w.std().item() - limit / math.sqrt(3)) <= 0.05 * limit / math.sqrt(3)


# ------------------------------------------------------------------------------------------------ the cases of the GPU edge tests
# tests/pgc_cases.py: every case is proven admissible here, with the float64 and the float32 restatement alone, so that
# tests/test_gpu_pgc_edges.py can hold the kernels to fixed bars without a "k x float32" band.
import pgc_cases as K


def test_case_table_covers_the_sizes():
    Ps, Bs = [c[2] for c in K.CASES], [c[1] for c in K.CASES]
    assert set(Ps) == {1, 3, 127, 128, 129, 255, 256, 257, 512, 513, 1025} and set(Bs) == {1, 2, 3}
    assert Bs.count(1) >= 3 and Bs.count(3) >= 3
    assert {c[0] for c in K.CASES} == {"init", "wide", "starved", "clamp", "dead"}
    starved = [P for r, _, P in K.CASES if r == "starved"]
    assert min(starved) < 128 and max(starved) > 512          # below one tile, above four


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_case_is_admissible(case):
    c = K.build(*case)
    ctx, grads, taps = K.reference(*case)
    want = K.quantities(c, ctx, grads, taps)
    for k, v in want.items():
        assert bool(torch.isfinite(v).all()), "float64 %s is not finite" % k
    for t in [c["x"], c["dout"]] + c["prm"]:
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    qs, n2, d = ctx["qs"][:, 0], ctx["n2"], ctx["d"]
    assert qs.min().item() >= 1e-30, "min qs %.3e" % qs.min().item()
    assert torch.sigmoid(c["prm"][1]).min().item() > 0.05                      # no variance near the sigmoid's underflow
    clamped = (d <= K.EPS).nonzero().tolist()
    if c["regime"] == "starved":
        got = qs[:, K.STARVED]
        assert K.BAND[0] <= got.min().item() and got.max().item() <= K.BAND[1], got.tolist()
        assert float(got.float().min()) > 0 and float((torch.sigmoid(c["prm"][1])[0, :, 0, K.STARVED] * got.float().min() ** 2).max()) == 0
    if c["regime"] == "clamp":
        sub, near, twin = c["sub"], c["near"], c["twin"]
        assert sorted(clamped) == sorted([list(t) for t in c["exact"]] + [list(sub[:3])]), clamped
        assert all(d[b, p, j].item() == 0 for b, p, j in c["exact"])
        assert 0 < d[sub[:3]].item() <= 0.9e-12 and 2e-12 <= d[near[:3]].item() <= 1e-11 and d[twin[:3]].item() > 1e-10
        assert sub[:2] == c["exact"][0][:2] and near[:2] == twin[:2]
        assert not any((b, p) == near[:2] for b, p, _ in clamped)              # the near-clamp column holds no clamped entry
        q = ctx["q"]
        b, p, j = c["exact"][1]
        assert q[b, p, j].item() > 1 - 1e-9                                      # a one-hot row
        assert abs(q[sub[:3]].item() - 0.5) < 1e-6 and abs(q[near[:3]].item() - 0.5) < 1e-3
        assert taps["dl"][sub[:3]].item() == 0 and abs(taps["dl"][near[:3]].item()) > 0.1
    else:
        assert clamped == []
    if c["regime"] == "dead":
        assert (n2 == 0).nonzero()[:, 1].tolist() == [K.DEAD] * c["B"] and bool((n2[:, K.DEAD] == 0).all())
        assert bool((ctx["zp"][:, K.DEAD] == 0).all())
        faint = n2[:, K.FAINT]
        assert K.FAINT_BAND[0] <= faint.min().item() and faint.max().item() <= K.FAINT_BAND[1], faint.tolist()
        assert ((n2 <= K.EPS).sum(1) == 2).all()
    else:
        assert n2.min().item() > 1e-3
    # the float32 restatement: the whole layer for everything judged norm-wise; dS and dqs, judged per vertex, from the float64
    # forward rounded to float32 -- what tests/test_gpu_pgc_edges.py hands the kernel that makes them.  (Through a float32
    # forward, per-vertex dqs is up to 1.2e-4 from float64: a sum over the channels that cancels, fed dzp with float32's error.)
    ctx32, grads32, taps32 = K.reference(*case, torch.float32)
    got = K.quantities(c, ctx32, grads32, taps32)
    got.update({k: K.staged32(*case)[k] for k in K.PER_VERTEX})
    dist = {k: K.distance(c, k, got[k], want[k]) for k in want}
    print(" ".join("%s %.1e" % kv for kv in sorted(dist.items(), key=lambda kv: -kv[1])[:6]), "min qs %.2e" % qs.min().item())
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    bad = {k: v for k, v in dist.items() if not v <= K.F32_BAR}
    assert not bad, bad


def test_far_inputs_are_not_admissible():
    """x scaled by 4: the float32 restatement leaves the bar, which is why no such case stands in the table"""
    c = K.build("wide", 2, 1025)
    x = 4 * c["x"]
    worst = 0.0
    res = {}
    for dt in (torch.float64, torch.float32):
        _, ctx = R.pgc_forward(x.to(dt), *(t.to(dt) for t in c["prm"]))
        res[dt] = R.pgc_backward(ctx, c["dout"].to(dt))
    for a, b in zip(res[torch.float32][:3], res[torch.float64][:3]):
        if bool(torch.isfinite(a).all()):
            worst = max(worst, K.rel_err(a, b))
        else:
            worst = float("inf")
    print("far: %.2e" % worst)
    assert worst > K.F32_BAR


def test_unstable_dqs_order_fails_on_the_starved_cases():
    """dzp S / (s qs qs) in float32 -- the order csrc/pgc.hip had -- is not finite on a starved case, and is the stable order's value
    in float64"""
    for case in [c for c in K.CASES if c[0] == "starved"]:
        ctx, _, taps = K.reference(*case)
        n2, n, zn, s, qs, S_ = ctx["n2"], ctx["n"], ctx["zn"], ctx["s"], ctx["qs"], ctx["S"]
        dzp = taps["dS"] * (s * qs)
        old64 = -(dzp * S_ / (s * qs * qs)).sum(1)
        assert K.per_vertex_err(old64, taps["dqs"]) < 1e-12
        f = lambda t: t.float()
        old32 = -(f(dzp) * f(S_) / (f(s) * f(qs) * f(qs))).sum(1)
        assert not bool(torch.isfinite(old32[:, K.STARVED]).all())
        assert bool(torch.isfinite(K.staged32(*case)["dqs"]).all())
