"""CPU: tests/tattn_reference.py, the float64 oracle of the TemporalAttention tests, is pinned here -- against the reference's literal
call (models/stgcn.py:75-85: transpose, reshape, Dense .., multiply, transpose) under torch autograd, and against central finite
differences in float64 -- and every case of tests/tattn_cases.py is shown to keep its hidden pre-activations away from the ReLU's kink,
so that float32 and float64 runs take the same ReLU pattern."""
import pytest
import torch

import tattn_cases as K
import tattn_reference as R
from util import rel_err

QUICK = [c for c in K.CASES if c[0] * c[1] * c[2] * c[3] <= 60000]


@pytest.mark.parametrize("case", QUICK, ids=K.case_id)
def test_restatement_is_the_literal_call_under_autograd(case):
    x, dout, params = K.make_case(case)
    out, ctx = R.forward(x, params)
    dx, grads, _ = R.backward(ctx, dout)
    leaves = [t.clone().requires_grad_() for t in [x] + params]
    lit = R.literal(leaves[0], leaves[1:])
    want = torch.autograd.grad(lit, leaves, dout)
    assert rel_err(out, lit) < 1e-13
    assert rel_err(dx, want[0]) < 1e-12
    for g, w in zip(grads, want[1:]):
        assert rel_err(g.reshape(w.shape), w) < 1e-12


def test_feature_index_is_v_major():
    """f[r, v C + c] = x[n, c, t, v]"""
    N, C, T, V = 2, 3, 4, 5
    x = torch.arange(N * C * T * V, dtype=torch.float64).reshape(N, C, T, V)
    f = R.features(x)
    for n, c, t, v in ((0, 0, 0, 0), (1, 2, 3, 4), (0, 1, 2, 3), (1, 0, 3, 2)):
        assert f[n * T + t, v * C + c] == x[n, c, t, v]


@pytest.mark.parametrize("case", [K.LISTED[0], K.LISTED[3], K.LISTED[7], (2, 3, 4, 5, (4, 3), 0)], ids=K.case_id)
def test_backward_against_central_differences(case):
    x, dout, params = K.make_case(case)
    _, ctx = R.forward(x, params)
    dx, grads, _ = R.backward(ctx, dout)
    loss = lambda xx, pp: (R.forward(xx, pp)[0] * dout).sum().item()
    gen = torch.Generator().manual_seed(1)
    eps = 1e-6
    for which, (t, g) in enumerate(zip([x] + params, [dx] + grads)):
        for _ in range(6):
            i = int(torch.randint(t.numel(), (1,), generator=gen))
            d = torch.zeros(t.numel(), dtype=torch.float64)
            d[i] = eps
            d = d.view(t.shape)
            plus, minus = [x] + params, [x] + params
            plus[which], minus[which] = t + d, t - d
            fd = (loss(plus[0], plus[1:]) - loss(minus[0], minus[1:])) / (2 * eps)
            got = g.reshape(-1)[i].item()
            assert abs(fd - got) <= 1e-6 * max(1.0, abs(got), g.abs().max().item()), (which, i, fd, got)


def test_need_dx_false_changes_no_parameter_gradient():
    x, dout, params = K.make_case(K.LISTED[0])
    _, ctx = R.forward(x, params)
    dx, grads, _ = R.backward(ctx, dout)
    none, grads2, _ = R.backward(ctx, dout, need_dx=False)
    assert none is None and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_hidden_pre_activations_stay_away_from_zero(case):
    """asserted on the float64 run alone: min |z| >= 1e-5 rms(z) per hidden layer (the float32 restatement rounds z to a few 1e-7 of
    the RMS), so no ReLU flips between the float32 kernels and the float64 oracle"""
    _, ref64, _ = K.reference(case)
    assert len(ref64["margins"]) == len(case[4])
    assert all(m >= 1e-5 for m in ref64["margins"]), ref64["margins"]
