"""The float64 restatements of tests/gin_reference.py (GraphIsoConv, GraphIsoConvTD): the TD one against oracle.stgin.graph_iso_conv
where the two overlap (filters = [h, h], K = 3), both against cases that can be worked out by hand and against a central finite
difference in `epsilon` (and torch.autograd.gradcheck in everything else)."""
import torch

import gin_reference as R
from oracle import stgin as O


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_td_restatement_agrees_with_the_oracle_in_training_and_inference():
    h, C, V = 6, 4, 5
    p = R.init_params([h, h], C, kernel_size=3, seed=1)
    x, A = _rand(2, C, 3, V, seed=2), _rand(2, V, V, seed=3)
    q = R.to_oracle(p)
    for training in (True, False):
        mine_stats, their_stats = {}, {}
        mine = R.graph_iso_conv_td(x, A, p, [h, h], 3, training=training, new_stats=mine_stats)
        theirs = O.graph_iso_conv(x, q, "l0.", A, training, their_stats, None, None)
        assert torch.allclose(mine, theirs, rtol=0, atol=1e-12)
        moved = R.to_oracle(dict(mine_stats, epsilon=p["epsilon"]))
        del moved["l0.epsilon"]
        assert set(moved) == set(their_stats) and (len(moved) == 12) == training      # 3 branches x 2 BatchNorms x (mean, var)
        for k, v in moved.items():
            assert torch.allclose(v, their_stats[k], rtol=0, atol=1e-13), k


def test_aggregation_with_an_empty_graph_is_the_scaled_input():
    """A = 0: the aggregation is (1 + epsilon) x; with a one-layer logits MLP the layer is the pointwise convolution of that"""
    C, V, f = 3, 5, 4
    p = R.init_params([f], C, return_logits=True, seed=4)
    x = _rand(2, C, V, seed=5)
    want = torch.einsum("ncv,cf->nfv", (1 + p["epsilon"]) * x, p["mlp.0.kernel"][0]) + p["mlp.0.bias"].view(1, -1, 1)
    got = R.graph_iso_conv(x, torch.zeros(2, V, V, dtype=torch.float64), p, [f], return_logits=True)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)


def test_aggregation_sums_the_neighbours_of_each_sample():
    """a binary A without self connections, another per sample: column w receives (1 + eps) x[w] plus its in-neighbours"""
    C, V = 2, 4
    x = _rand(2, C, V, seed=6)
    A = torch.zeros(2, V, V, dtype=torch.float64)
    A[0, 0, 1] = A[0, 2, 1] = A[1, 3, 0] = 1.0
    p = {"epsilon": torch.tensor(0.25, dtype=torch.float64), "mlp.0.kernel": torch.eye(C, dtype=torch.float64)[None],
         "mlp.0.bias": torch.zeros(C, dtype=torch.float64)}
    out = R.graph_iso_conv(x, A, p, [C], return_logits=True)
    want = 1.25 * x
    want[0, :, 1] += x[0, :, 0] + x[0, :, 2]
    want[1, :, 0] += x[1, :, 3]
    assert torch.allclose(out, want, rtol=0, atol=1e-14)


def test_td_slices_go_through_their_own_mlp():
    """A_0 = 2 I and epsilon = 0.5: slice 0 sees 2 x, the self slice 1.5 x; zeroing one branch's last gamma and beta removes exactly
    that branch, and what is left is the other branch's MLP on its own slice"""
    C, V, h = 3, 4, 5
    p = R.init_params([h], C, kernel_size=2, seed=7)
    p["epsilon"] = torch.tensor(0.5, dtype=torch.float64)
    x, A = _rand(2, C, 3, V, seed=8), 2.0 * torch.eye(V, dtype=torch.float64)[None]
    for gone, scale in ((1, 2.0), (0, 1.5)):
        q = {k: (torch.zeros_like(v) if k in ("mlps.%d.0.gamma" % gone, "mlps.%d.0.beta" % gone) else v) for k, v in p.items()}
        left = R._mlp(scale * x, p, "mlps.%d." % (1 - gone), [h], False, True, True, None, None)
        assert torch.allclose(R.graph_iso_conv_td(x, A, q, [h], 2), left, rtol=0, atol=1e-13)


def _central_difference(fn, p, w, h=1e-6):
    lo, hi = dict(p), dict(p)
    lo["epsilon"], hi["epsilon"] = p["epsilon"] - h, p["epsilon"] + h
    return (((fn(hi) - fn(lo)) * w).sum() / (2 * h)).item()


def test_epsilon_gradient_against_a_central_difference():
    C, V = 3, 5
    x3, A3, x4, A4 = _rand(2, C, V, seed=9), _rand(2, V, V, seed=10), _rand(2, C, 3, V, seed=11), _rand(2, V, V, seed=12)
    cases = [(R.init_params([6, 4], C, seed=13), lambda q: R.graph_iso_conv(x3, A3, q, [6, 4])),
             (R.init_params([6, 4], C, return_logits=True, seed=14), lambda q: R.graph_iso_conv(x3, A3, q, [6, 4], return_logits=True)),
             (R.init_params([4, 4], C, kernel_size=3, seed=15), lambda q: R.graph_iso_conv_td(x4, A4, q, [4, 4], 3))]
    for p, fn in cases:
        leaf = dict(p)
        leaf["epsilon"] = p["epsilon"].clone().requires_grad_(True)
        out = fn(leaf)
        w = _rand(*out.shape, seed=16)
        got, = torch.autograd.grad((out * w).sum(), leaf["epsilon"])
        want = _central_difference(fn, p, w)
        assert abs(got.item() - want) <= 1e-6 * max(1.0, abs(want)), (got.item(), want)


def test_gradients_against_finite_differences():
    C, V = 3, 4
    for td in (False, True):
        p = R.init_params([4, 3], C, kernel_size=3 if td else None, seed=17)
        names = [k for k in sorted(p) if "moving" not in k]
        x = (_rand(2, C, 2, V, seed=18) if td else _rand(2, C, V, seed=18)).requires_grad_(True)
        A = _rand(2, V, V, seed=19).requires_grad_(True)

        def fn(x, A, *vals):
            q = dict(p)
            q.update(zip(names, vals))
            return R.graph_iso_conv_td(x, A, q, [4, 3], 3) if td else R.graph_iso_conv(x, A, q, [4, 3])
        assert torch.autograd.gradcheck(fn, (x, A) + tuple(p[k].clone().requires_grad_(True) for k in names))
