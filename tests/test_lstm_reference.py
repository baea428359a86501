"""tests/lstm_reference.py (the yardstick of tests/test_gpu_lstm_sampler.py) pinned two ways on the CPU: against torch.nn.LSTM in
float64 (the same gate order i, f, g, o; weight_ih = kernel^T, weight_hh = recurrent_kernel^T, bias_ih = bias, bias_hh = 0), and
against a case small enough to work out by hand (T = 2, u = 1, scalars)."""
import math

import torch

import lstm_reference as R


def _params(widths, F0, g, dtype=torch.float64):
    out, F = [], F0
    for u in widths:
        out.append((torch.randn(F, 4 * u, generator=g, dtype=dtype) * 0.4, torch.randn(u, 4 * u, generator=g, dtype=dtype) * 0.4,
                    torch.randn(4 * u, generator=g, dtype=dtype) * 0.3))
        F = u
    return out


def test_stack_matches_torch_nn_lstm_float64():
    g = torch.Generator().manual_seed(11)
    N, T, F0, widths = 3, 9, 7, [6, 4]
    params = _params(widths, F0, g)
    x = torch.randn(N, T, F0, generator=g, dtype=torch.float64)
    want, F = x, F0
    for (kernel, rec, bias), u in zip(params, widths):
        m = torch.nn.LSTM(F, u, batch_first=True).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(kernel.t()), m.weight_hh_l0.copy_(rec.t()), m.bias_ih_l0.copy_(bias), m.bias_hh_l0.zero_()
            want = m(want)[0]
        F = u
    got = R.lstm_stack(x, params)
    assert got.shape == (N, T, widths[-1])
    assert (got - want).abs().max().item() < 1e-12


def test_layer_returns_its_state():
    g = torch.Generator().manual_seed(12)
    (kernel, rec, bias), = _params([3], 4, g)
    x = torch.randn(2, 5, 4, generator=g, dtype=torch.float64)
    h, gates, c = R.lstm_layer(x, kernel, rec, bias, return_state=True)
    assert torch.equal(h, R.lstm_layer(x, kernel, rec, bias))
    assert gates.shape == (2, 5, 12) and c.shape == (2, 5, 3)
    assert torch.allclose(h, gates[:, :, 9:] * torch.tanh(c), atol=0, rtol=0)


def test_hand_computed_two_steps_one_unit():
    """F = 1, u = 1: every quantity is a scalar"""
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    x0, x1 = 0.5, -1.25
    wi, wf, wg, wo = 0.3, -0.2, 0.7, 0.1
    ui, uf, ug, uo = -0.4, 0.6, 0.2, -0.5
    bi, bf, bg, bo = 0.05, 1.0, -0.1, 0.2
    i0, f0, g0, o0 = sig(x0 * wi + bi), sig(x0 * wf + bf), math.tanh(x0 * wg + bg), sig(x0 * wo + bo)
    c0 = i0 * g0                      # f0 * 0 + i0 g0
    h0 = o0 * math.tanh(c0)
    i1, f1 = sig(x1 * wi + h0 * ui + bi), sig(x1 * wf + h0 * uf + bf)
    g1, o1 = math.tanh(x1 * wg + h0 * ug + bg), sig(x1 * wo + h0 * uo + bo)
    c1 = f1 * c0 + i1 * g1
    h1 = o1 * math.tanh(c1)
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    h = R.lstm_layer(t(x0, x1).view(1, 2, 1), t(wi, wf, wg, wo).view(1, 4), t(ui, uf, ug, uo).view(1, 4), t(bi, bf, bg, bo))
    assert h.shape == (1, 2, 1)
    assert abs(h[0, 0, 0].item() - h0) < 1e-15 and abs(h[0, 1, 0].item() - h1) < 1e-15
    assert f0 > 0.5 and h0 != h1      # (the case is not degenerate)


def test_sampler_order_gather_scale_and_gradients():
    g = torch.Generator().manual_seed(13)
    N, C, T, V, k = 2, 2, 6, 3, 4
    params = [tuple(p.requires_grad_(True) for p in layer) for layer in _params([3, 1], V * C, g)]
    x = torch.randn(N, C, T, V, generator=g, dtype=torch.float64, requires_grad=True)
    out, scores, idx = R.temporal_sampler(x, params, k)
    assert out.shape == (N, C, k, V) and scores.shape == (N, T) and idx.shape == (N, k)
    for n in range(N):
        picked = scores[n, idx[n]]
        assert bool((picked[:-1] >= picked[1:]).all()) and len(set(idx[n].tolist())) == k
        assert picked[-1] >= max(scores[n, t] for t in range(T) if t not in idx[n].tolist())
        for j in range(k):
            assert torch.equal(out[n, :, j], x[n, :, idx[n, j]] * scores[n, idx[n, j]])
    # the selection may be imposed; the scale is still the function's own score there
    other = torch.tensor([[5, 0, 1, 2], [3, 3, 4, 0]])
    out2 = R.temporal_sampler(x, params, k, indices=other)[0]
    assert torch.equal(out2[1, :, 1], x[1, :, 3] * scores[1, 3])
    grads = torch.autograd.grad(out.sum(), [x] + [p for layer in params for p in layer])
    assert all(bool(torch.isfinite(gr).all()) and gr.abs().max() > 0 for gr in grads)


def test_stable_topk_breaks_ties_by_ascending_index():
    s = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0, 1.0]])
    values, idx = R.stable_topk(s, 5)
    assert idx.tolist() == [[1, 2, 4, 0, 5]] and values.tolist() == [[3.0, 3.0, 3.0, 1.0, 1.0]]
